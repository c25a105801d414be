"""The ten kernels of csrc/state.hip -- the constraint, state and z-assembly stages between the recognition network and the recursion,
and the ELBO assembly behind it -- against the float64 oracle at EVERY object count stove_supair_state_fwd2 accepts (1 .. 8), at
eight (n, T, skip) shapes that each hit one edge (helpers.STATE_SHAPES), with 'greedy' and 'volatile' at every count and '3_only' at
three, the smoothing stencil on and off.  Where tests/test_gpu_dynamics.py::test_state_pipeline_against_torch_chain and
test_elbo_assembly_against_torch compare one single-workgroup shape with this project's own float32 PyTorch chain, the reference here is
helpers.state_chain / zall_chain / elbo_chain: the oracle's constrain_zp, matchers, fix_supair, v_from_state, v_std_from_pos,
sy_from_quotient and normal_log_prob in float64, pinned to the reference's recorded results by tests/test_state_chain_cpu.py.

1. stage by stage through the C ABI (ctypes, every output buffer pre-filled with nan: nothing may stay unwritten);
2. ops.supair_state / ops.zall / ops.elbo with autograd, every combination of absent output gradients the training step can produce;
3. skip = 1: the recursion starts from the zero row of v_from_state, and Stove.forward agrees with its op-by-op chain.

Inputs: float64 draws rounded to float32, so that both sides see the same numbers; chosen per sequence on the CPU (helpers.state_inputs)
such that no |jump| lies within 1e-4 of fix_supair's threshold and every matcher decision wins by more than 1e-5 -- asserted again
here on the reference side before anything is compared.

Bars: what the project holds for these operations at its one shape -- 1e-6 state values, 1e-5 the gradient of the codes and the
ELBO's gradients, at every case, as they stand; 1e-5 relative the ELBO and its two statistics, except where the float64
chain's own float32 run is further than 1e-5 / 6 from its float64 run: there 6 x that gap (gpu_helpers.regime_bar).  That happens where
a mean of a few log-densities of either sign nearly cancels -- the ELBO at one object and log q at five, both at (1, 3, 2): gaps
5.0e-6 -- not at the long sums of (2, 100, 2) and (300, 3, 2).  The chain's float32 gap is printed next to every achieved error.
The z assembly is one product per element each way: 1e-6 there, forward and backward (three float32 roundings are
2e-7).  Achieved errors: profiles/state_parity.json."""
import ctypes

import pytest
import torch

import stove_oracle as O
from gpu_helpers import check, err, regime_bar
from helpers import (STATE_COUNTS, STATE_IDX_FORMS, STATE_MATCHERS, STATE_SHAPES, assert_state_conditions, assert_state_coverage,
                     elbo_chain, elbo_inputs, gather_slots, given_idx_inputs, match_walk, source_index, state_case_id, state_cases,
                     state_chain, state_config, state_coverage, state_inputs, state_last_stage, state_reference, state_span_low,
                     zall_chain, FIX_CLEARANCE, FIX_THRESHOLD)
from test_gpu_dynamics import make_cfg

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
L = 12                                   # the unstructured latents of the recursion's initial state at cl = 32
CASES = state_cases()
NAN = float('nan')


def _dev(t, grad=False):
    return None if t is None else t.float().to(DEV).requires_grad_(grad)


def _key(o, n, T, skip, what):
    return f'state.o{o}.n{n}T{T}s{skip}.{what}'


def _held(key, got, want, low, bar):
    """check(got against the float64 chain's `want`) at `bar`; what the chain's own float32 run `low` differs from `want` by is
    printed next to the achieved error"""
    e, gap = err(got, want), err(low, want)
    print(f'{key}: {e:.3g} (chain f32 gap {gap:.3g}, bar {bar:.3g})')
    check(key, e, bar)


def _noise(seed, n, o):
    return torch.randn(n, o, L, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).float().double()


def _fwd2(c, n, T, o, skip, fix, mode='greedy', codes=None, zc=None, idx=None, noise=None):
    """stove_supair_state_fwd2 through the ctypes binding, nothing of ops in between.  codes (M, 8): the full entry; codes None: the
    last stage alone on the caller's zc and idx.  Every output starts as nan (hits 255, idx -1) and must come back written."""
    from stove_amd import _lib
    from stove_amd.ops import MATCH_MODES
    lib, p = _lib.load(), _lib.ptr
    full = lambda *s: torch.full(s, NAN, device=DEV)          # noqa: E731
    out = {'zfix': full(n, T, o, 8), 'hits': torch.full((n, T, o), 255, dtype=torch.uint8, device=DEV), 'zl': full(n, T - skip, o, 6),
           'sl': full(n, T - skip, o, 6), 'init': full(n, o, 6 + (L if noise is not None else 0))}
    if codes is not None:
        out.update(zc=full(n, T, o, 8), pos=full(n, T, o, 2), idx=torch.full((n, T, o), -1, dtype=torch.int64, device=DEV))
        kc = (ctypes.c_float * 16)(*state_span_low(c))
    else:
        out.update(zc=zc.contiguous(), pos=None, idx=idx.contiguous())
        kc = None
    _lib.check(lib.stove_supair_state_fwd2(p(codes), kc, p(out['zc']), p(out['pos']), p(out['idx']), p(out['zfix']), p(out['hits']),
                                           p(out['zl']), p(out['sl']), p(out['init']), out['init'].shape[-1], p(noise),
                                           L if noise is not None else 0, n, T, o, skip, int(fix), MATCH_MODES[mode], _lib.stream()),
               'stove_supair_state_fwd2')
    torch.cuda.synchronize()
    for k, v in out.items():
        if v is not None and v.is_floating_point():
            assert not torch.isnan(v).any(), k + ' holds elements the kernels did not write'
    assert int(out['hits'].max()) <= 3 and int(out['idx'].min()) >= 0 and int(out['idx'].max()) < o
    return out


# ------------------------------------------------------------------------------------------------ 1. stage by stage through the C ABI
@pytest.mark.parametrize('o', STATE_COUNTS)
def test_constraint_stage_over_the_sigmoid_tails(o):
    """1a. zp_constrain_k on codes spread evenly over [-6, 6] in every dim (n T o 8 = 280 o elements: never a multiple of the
    workgroup), against O.constrain_zp; pos is the copy of the two position columns"""
    n, T = 5, 7
    c = state_config(o)
    g = torch.Generator().manual_seed(100 + o)
    codes = (torch.rand(n * T * o, 8, generator=g, dtype=torch.float64) * 12 - 6).float().double()
    codes[0], codes[-1] = -6.0, 6.0
    got = _fwd2(c, n, T, o, 2, True, 'volatile', codes=_dev(codes))
    want, low = torch.cat(O.constrain_zp(c, codes), -1), torch.cat(O.constrain_zp(c, codes.float()), -1)
    _held(_key(o, n, T, 2, 'zc'), got['zc'].view(-1, 8), want, low, 1e-6)
    for d in range(8):              # column by column: the scale stds are three orders below the positions
        _held(_key(o, n, T, 2, 'zc.col'), got['zc'].view(-1, 8)[:, d], want[:, d], low[:, d], 1e-6)
    assert torch.equal(got['pos'], got['zc'][..., 2:4])


@pytest.mark.parametrize('case', CASES, ids=state_case_id)
def test_constraint_and_matching_inside_the_pipeline(case):
    """1a / 1c. The full entry: zc and pos against O.constrain_zp, and idx EXACTLY the index the oracle's matcher takes in float64
    on the device's own positions (float32 values lifted exactly), recovered from its output by helpers.source_index"""
    o, n, T, skip, mode, fix = case
    c = state_config(o, skip)
    ref = state_reference(case)
    assert_state_conditions(ref, mode)
    codes = state_inputs(case).reshape(-1, 8)
    got = _fwd2(c, n, T, o, skip, fix, mode, codes=_dev(codes))
    low = torch.cat(O.constrain_zp(c, codes.float()), -1).view(n, T, o, 8)
    _held(_key(o, n, T, skip, 'zc'), got['zc'], ref['zc'], low, 1e-6)
    assert torch.equal(got['pos'], got['zc'][..., 2:4])
    zc = got['zc'].double().cpu()
    zm, sm, _ = STATE_MATCHERS[mode](c, zc[..., :4], zc[..., 4:], None)
    idx = source_index(zc, torch.cat([zm, sm], -1), 1e-9)
    assert torch.equal(idx, match_walk(got['pos'].double().cpu(), mode)[0])
    assert torch.equal(got['idx'].cpu(), idx)
    assert torch.equal(idx, ref['idx'])                      # (the margins make it the reference's own, too)
    assert torch.equal(got['hits'].cpu().long(), ref['hits'])


GIVEN = [(o, si, form) for o in STATE_COUNTS for si in range(len(STATE_SHAPES)) for form in STATE_IDX_FORMS if form != 'volatile' or o >= 2]


@pytest.mark.parametrize('o,si,form', GIVEN, ids=lambda v: v if isinstance(v, str) else str(v))
def test_last_stage_alone_on_a_given_matching(o, si, form):
    """1b. codes == NULL: the caller's zc and idx, supair_state_fwd_k alone.  idx: the identity, a random permutation per frame, and
    per-frame non-permutations (one object twice, one left out -- what 'volatile' produces) at every o >= 2.  The hits byte is
    exactly the chain's two-bit mask; zfix, zl, sl and the initial state hold 1e-6 at both row strides (6, and 6 + 12 with the
    latent draws), bit for bit the same at both; the latent part is 0.01f x the draw, bit for bit; rows the stencil leaves alone
    are copies.  The stencil is off on a quarter of the cases."""
    n, T, skip = STATE_SHAPES[si]
    fix = (o + si) % 4 != 0
    zc, idx = given_idx_inputs(o, n, T, form, 40000 + 1000 * o + 10 * si + STATE_IDX_FORMS.index(form))
    zm = gather_slots(zc, idx)
    noise = _noise(o + si, n, o)
    want, low = state_last_stage(zm, skip, fix, noise), state_last_stage(zm.float(), skip, fix, noise.float())
    assert float((want['jump'] - FIX_THRESHOLD).abs().min()) > FIX_CLEARANCE
    c = state_config(o, skip)
    zc_d, idx_d, noise_d = _dev(zc), idx.to(DEV), _dev(noise)
    g6 = _fwd2(c, n, T, o, skip, fix, zc=zc_d, idx=idx_d)
    g18 = _fwd2(c, n, T, o, skip, fix, zc=zc_d, idx=idx_d, noise=noise_d)
    assert torch.equal(g6['hits'].cpu().long(), want['hits']) and torch.equal(g18['hits'], g6['hits'])
    for k in ('zfix', 'zl', 'sl'):
        assert torch.equal(g6[k], g18[k]), k
        _held(_key(o, n, T, skip, 'given.' + k), g6[k], want[k], low[k], 1e-6)
    assert g6['init'].shape == (n, o, 6) and g18['init'].shape == (n, o, 6 + L) and torch.equal(g18['init'][..., :6], g6['init'])
    assert torch.equal(g18['init'][..., 6:], 0.01 * noise_d)
    if skip == 1:
        assert not g6['init'].any() and not want['init'][..., :6].any()
    else:
        _held(_key(o, n, T, skip, 'given.init'), g6['init'], want['init'][..., :6], low['init'][..., :6], 1e-6)
    plain = (g6['hits'] == 0).unsqueeze(-1).expand(-1, -1, -1, 8)
    assert torch.equal(g6['zfix'][plain], gather_slots(zc_d, idx_d)[plain])
    assert fix or not g6['hits'].any()


def test_grid_coverage():
    """over the grid the references show every hit mask, runs of smoothed frames, a smoothed frame at t = skip - 1 and at t = skip, and
    a non-permutation of 'volatile' at every o >= 2"""
    assert_state_coverage(state_coverage(CASES))


# ------------------------------------------------------------------------------------------------ 2. through ops, with autograd
GRAD_SETS = {'all': (0, 1, 2, 3), 'zfix': (0,), 'zl': (1,), 'sl': (2,), 'init': (3,), 'zl+init': (1, 3)}


def _state_chain_with_grads(c, codes, noise, ws, n, T, o, skip, fix, mode, dtype):
    x = codes.to(dtype).clone().requires_grad_()
    r = state_chain(c, x, n, T, o, skip, fix, mode, noise.to(dtype))
    outs = [r['zfix'], r['zl'], r['sl'], r['init']]
    grads = {}
    for name, use in GRAD_SETS.items():
        loss = sum((outs[i] * ws[i].to(dtype)).sum() for i in use)
        # (skip = 1: the initial state is a constant, a loss over it alone depends on no code)
        g = torch.autograd.grad(loss, x, retain_graph=True, allow_unused=True)[0] if loss.requires_grad else None
        grads[name] = torch.zeros_like(x) if g is None else g
    return {k: (v.detach() if torch.is_tensor(v) else v) for k, v in r.items()}, grads


@pytest.mark.parametrize('case', CASES, ids=state_case_id)
def test_supair_state_against_the_chain(case):
    """ops.supair_state, forward (all five outputs; idx exactly) and backward into the codes.  Loss: every output under a random weight
    of its own, summed (test_state_pipeline_against_torch_chain's) -- over all four differentiable outputs, over EACH of them alone
    and over zl + init (a loss without the scene term): _SupairStateFn hands the kernel a null pointer for every output nothing
    differentiates, so these run the null branches of g6_at and supair_gfix.  Bars: 1e-6 the values, 1e-5 the gradient.  At skip = 1
    the initial state is a constant: its weight contributes an exactly zero gradient.  Every backward runs twice: bit for bit the
    same.  Without the latent draws (row stride 6) values and gradient are bit for bit those of the stride-18 call."""
    from stove_amd import ops
    o, n, T, skip, mode, fix = case
    c = state_config(o, skip)
    codes = state_inputs(case).reshape(-1, 8)
    noise = _noise(7 * o + n, n, o)
    g = torch.Generator().manual_seed(50000 + CASES.index(case))
    ws = [torch.randn(*s, generator=g, dtype=torch.float64).float().double()
          for s in ((n, T, o, 8), (n, T - skip, o, 6), (n, T - skip, o, 6), (n, o, 6 + L))]
    want, gwant = _state_chain_with_grads(c, codes, noise, ws, n, T, o, skip, fix, mode, torch.float64)
    low, glow = _state_chain_with_grads(c, codes, noise, ws, n, T, o, skip, fix, mode, torch.float32)
    assert_state_conditions(want, mode)

    def run(lat):
        x = _dev(codes, True)
        outs = ops.supair_state(x, state_span_low(c), n, T, o, skip, fix, mode, lat_noise=lat)
        wd = [_dev(w) for w in ws]
        if lat is None:
            wd[3] = wd[3][..., :6].contiguous()
        grads = {}
        for name, use in GRAD_SETS.items():
            loss = sum((outs[i] * wd[i]).sum() for i in use)
            a, = torch.autograd.grad(loss, x, retain_graph=True)
            b, = torch.autograd.grad(loss, x, retain_graph=True)
            assert torch.equal(a, b), name
            grads[name] = a
        return outs, grads

    outs, grads = run(_dev(noise))
    key = lambda what: _key(o, n, T, skip, what)          # noqa: E731
    for name, t in zip(('zfix', 'zl', 'sl', 'init'), outs):
        assert t.shape == want[name].shape and not torch.isnan(t).any(), name
        _held(key(name), t, want[name], low[name], 1e-6)
    assert torch.equal(outs[3][..., 6:], 0.01 * _dev(noise))
    assert torch.equal(outs[4].cpu(), want['idx'])
    for name in GRAD_SETS:
        assert not torch.isnan(grads[name]).any(), name
        _held(key('grad_codes.' + name), grads[name], gwant[name], glow[name], 1e-5)
    if skip == 1:
        assert not outs[3][..., :6].any() and not gwant['init'].any() and not grads['init'].any()
    outs6, grads6 = run(None)
    assert outs6[3].shape == (n, o, 6) and torch.equal(outs6[3], outs[3][..., :6])
    for a, b in zip(outs6[:3] + (outs6[4],), outs[:3] + (outs[4],)):
        assert torch.equal(a, b)
    for name in GRAD_SETS:
        assert torch.equal(grads6[name], grads[name]), name


def _poison(*like):
    """best effort: leave nan in the caching allocator's free blocks of the sizes the next call asks for"""
    junk = [torch.full_like(t, NAN) for t in like]
    del junk


ZALL = [(o, si) for o in STATE_COUNTS for si in range(len(STATE_SHAPES))]


@pytest.mark.parametrize('o,si', ZALL)
def test_zall_against_the_chain(o, si):
    """ops.zall: forward against cat([z_sup[:, 1:skip], z_s[..., :4]]) -> sy_from_quotient, and the backward into zfix and zs when only
    the first output is used (dz_in null), when both are (the pass-through's gradient is added in the kernel), and when only the
    pass-through is (no launch: the gradient is handed on as it came).  zall_bwd_k promises to write every element of both
    gradients: the allocator's free blocks are filled with nan just before, and none may show; where the chain's gradient is an
    exact zero (frame 0, frames from skip on, the std columns of zfix) so is the kernel's.  Bar 1e-6 throughout."""
    from stove_amd import ops
    n, T, skip = STATE_SHAPES[si]
    g = torch.Generator().manual_seed(60000 + 10 * o + si)
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64).float().double()          # noqa: E731
    zfix, zs = r(n, T, o, 8) * 1.6 - 0.8, r(n, T - skip, o, 18) * 1.6 - 0.8
    w, w2 = r(n * (T - 1) * o, 4) * 2 - 1, r(n, T - skip, o, 18) * 2 - 1

    def chain(dtype):
        a, b = zfix.to(dtype).requires_grad_(), zs.to(dtype).requires_grad_()
        z = zall_chain(a, b, skip)
        first, both = (z * w.to(dtype)).sum(), (z * w.to(dtype)).sum() + (b * w2.to(dtype)).sum()
        grads = [torch.autograd.grad(loss, (a, b), retain_graph=True, allow_unused=True) for loss in (first, both)]
        return [z.detach()] + [[torch.zeros_like(t) if g is None else g for g, t in zip(gs, (a, b))] for gs in grads]
    want, low = chain(torch.float64), chain(torch.float32)
    a, b = _dev(zfix, True), _dev(zs, True)
    z, through = ops.zall(a, b, n, T, o, skip)
    key = lambda what: _key(o, n, T, skip, 'zall.' + what)          # noqa: E731
    assert z.shape == want[0].shape and torch.equal(through, b)
    _held(key('z'), z, want[0], low[0], 1e-6)
    wd, w2d = _dev(w), _dev(w2)
    for i, (name, loss) in enumerate((('first', (z * wd).sum()), ('both', (z * wd).sum() + (through * w2d).sum())), 1):
        res = []
        for _ in range(2):
            _poison(a, b)
            res.append(torch.autograd.grad(loss, (a, b), retain_graph=True))
        for j, t in enumerate(('zfix', 'zs')):
            assert torch.equal(res[0][j], res[1][j]) and not torch.isnan(res[0][j]).any(), (name, t)
            _held(key(f'grad_{t}.{name}'), res[0][j], want[i][j], low[i][j], 1e-6)
            assert not res[0][j][(want[i][j] == 0).to(DEV)].any(), (name, t)
    ga, gb = torch.autograd.grad((through * w2d).sum(), (a, b), allow_unused=True)
    assert ga is None and torch.equal(gb, w2d)


_TSTD = {}


def _tstd(which):
    """'mixed': the stds of test_elbo_assembly_against_torch; 'model': Dynamics.transition_lik_std_host, what Stove.forward passes"""
    if which == 'mixed':
        return [0.01] * 4 + [0.02] * 12
    if 'model' not in _TSTD:
        from stove_amd.video_prediction.dynamics import Dynamics
        _TSTD['model'] = list(Dynamics(make_cfg()).transition_lik_std_host)
        assert _TSTD['model'] == [float(v) for v in O.transition_std(state_config(3))]
    return _TSTD['model']


def _rel(a, b):
    a, b = (float(t.detach()) if torch.is_tensor(t) else float(t) for t in (a, b))
    return abs(a - b) / abs(b)


@pytest.mark.parametrize('which', ['mixed', 'model'])
@pytest.mark.parametrize('o,si', ZALL)
def test_elbo_against_the_chain(o, si, which):
    """ops.elbo: the scalar and both statistics against helpers.elbo_chain in float64 (1e-5 relative), stds of q down to 0.05; at
    skip = 1 the mean over the empty set of SuPAIR-scored frames counts 0, as elbo_final_k states.  (2, 100, 2) takes elbo_part_k's
    row loop round a second time from three objects on, (300, 3, 2) elbo_final_k's sequence loop.  Gradients of all five inputs under
    an upstream gradient of -0.7 (1e-5), the two constants of g_lik each on its own side of skip - 1; two backward runs agree bit
    for bit.  The bar of the three scalars is regime_bar(1e-5, gap of the float32 chain on the same inputs): a mean of log-densities that
    nearly cancels cannot be held to 1e-5 of itself by any float32 evaluation; the gradients' bars are the plain 1e-5."""
    from stove_amd import ops
    n, T, skip = STATE_SHAPES[si]
    tstd = _tstd(which)
    ins = elbo_inputs(torch.Generator().manual_seed(70000 + 10 * o + si), n, T, o, skip, tstd)
    assert float(ins[2].min()) == float(torch.tensor(0.05).float())
    up = -0.7

    def chain(dtype):
        leaves = [t.to(dtype).requires_grad_() for t in ins]
        vals = elbo_chain(*leaves, tstd, skip)
        return [v.detach() for v in vals], torch.autograd.grad(up * vals[0], leaves)
    (want, gwant), (low, glow) = chain(torch.float64), chain(torch.float32)
    leaves = [_dev(t, True) for t in ins]
    elbo, stats = ops.elbo(*leaves, tstd, n, T, o, skip)
    key = lambda what: _key(o, n, T, skip, 'elbo.' + what)          # noqa: E731
    for name, got, w, lo in zip(('value', 'trans', 'logq'), (elbo, stats[0], stats[1]), want, low):
        e, gap = _rel(got, w), _rel(lo, w)
        print(f'{key(name)}: {e:.3g} (chain f32 gap {gap:.3g}, bar {regime_bar(1e-5, gap):.3g})')
        check(key(name), e, regime_bar(1e-5, gap))
    got = torch.autograd.grad(up * elbo, leaves, retain_graph=True)
    again = torch.autograd.grad(up * elbo, leaves)
    for name, a, b, w, lo in zip(('zs', 'mean', 'std', 'zdyn', 'lik'), got, again, gwant, glow):
        assert torch.equal(a, b) and not torch.isnan(a).any(), name
        _held(key('grad_' + name), a, w, lo, 1e-5)
    glik = got[4]
    if skip > 1:
        _held(key('grad_lik.sup'), glik[:, :skip - 1], gwant[4][:, :skip - 1], glow[4][:, :skip - 1], 1e-5)
        assert _rel(glik[0, 0], up / (n * (skip - 1))) < 1e-6
    _held(key('grad_lik.step'), glik[:, skip - 1:], gwant[4][:, skip - 1:], glow[4][:, skip - 1:], 1e-5)
    assert _rel(glik[-1, -1], up / (n * (T - skip))) < 1e-6


# ------------------------------------------------------------------------------------------------ 3. skip = 1 through the model
def test_stove_forward_at_skip_one_fused_state_on_and_off():
    """Stove.forward with skip = 1 under injected noise: the fused state pipeline (which now writes the zero initial state itself) and
    the op-by-op chain give the same ELBO, and both are finite"""
    from gpu_helpers import fill_analytic
    from stove_amd.video_prediction.stove import Stove
    n, T = 2, 4
    g = torch.Generator().manual_seed(13)
    x = (torch.rand(n, T, 3, 32, 32, generator=g) < 0.04).float().to(DEV)
    noise = {}

    def noise_fn(kind, shape):
        key = (kind, tuple(shape))
        if key not in noise:
            noise[key] = torch.randn(*shape, generator=g)
        return noise[key]
    elbos = []
    for fused in (True, False):
        st = fill_analytic(Stove(make_cfg(skip=1, fused_state=fused, debug_match_objects='greedy'))).to(DEV)
        st.noise_fn = noise_fn
        elbo, _, _ = st(x, 0, None)
        (-elbo).backward()
        assert all(bool(torch.isfinite(p.grad).all()) for p in st.parameters() if p.grad is not None)
        elbos.append(float(elbo.detach()))
    assert all(e == e and abs(e) < float('inf') for e in elbos), elbos
    check('state.skip1.stove_elbo', abs(elbos[0] - elbos[1]) / abs(elbos[1]), 1e-5)
