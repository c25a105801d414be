"""The kernels that open and close every training step -- spn_bake_k / spn_bake_bwd_k, arena_gather_k / arena_scatter_add_k, grad_scan_k /
flat_adam_k / adam_tick_k, bw_transform_k / bw_transform_u8_k (csrc/arena.hip) and noise_normal_k (csrc/state.hip) -- through their C
entry points (stove_amd._lib), against the float64 references of tests/arena_cases.py, which tests/test_arena_cases_cpu.py pins and whose
input conditions it asserts.  Every output starts as NaN or a pattern, every call runs twice and the two runs must be bit-equal; the
achieved errors are recorded under arena.<kernel>.<case>.<quantity> (gpu_helpers.check / check_ratio; tests/conftest.py writes them out
at the end of the session; committed: profiles/arena_parity.json).

Bars (arena_cases): table values 1e-6 and table gradients 1e-5, FlatAdam 1e-6 -- or 6 x the reference's own float32 gap on the same case
under the same error function where that is larger (regime_bar), measured on the CPU inside the test; gather, scatter and both
bw_transform kernels are exact; the noise generator lies within arena_cases.noise_bar() of the numpy Philox + Box-Muller reference."""
import ctypes

import numpy as np
import pytest
import torch

import arena_cases as A
from gpu_helpers import check, check_ratio, err, err_l2, err_small

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN = float('nan')
GUARD = 64
INVALID = 1                         # hipErrorInvalidValue


def _L():
    from stove_amd import _lib
    return _lib, _lib.load()


def _dev(a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(DEV).contiguous()


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    a = _np(a) if torch.is_tensor(a) else np.asarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else a.dtype)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------------------------ 1. table bake
def _device_plan(arena):
    """the arena's SPN index plan with its tables on the device -> (plan struct, what keeps the tables alive)"""
    _lib, _ = _L()
    keep = {k: _dev(v) for k, v in arena._spn['keep'].items()}
    src, plan = arena._spn['plan'], _lib.SpnArenaPlan()
    for k, v in keep.items():
        assert v.dtype == torch.int32
        setattr(plan, k, v.data_ptr())
    for k in ('obj_root', 'bg_root', 'obj_vmin', 'obj_vmax', 'bg_vmin', 'bg_vmax'):
        setattr(plan, k, getattr(src, k))
    return plan, keep


def _bake(data, plan):
    _lib, lib = _L()
    buf = torch.full((sum(A.TABLE_FLOATS) + GUARD,), NAN, device=DEV)
    tabs = torch.split(buf, list(A.TABLE_FLOATS) + [GUARD])
    _lib.check(lib.stove_spn_bake(data.data_ptr(), ctypes.byref(plan), *[t.data_ptr() for t in tabs[:5]], _lib.stream()), 'stove_spn_bake')
    torch.cuda.synchronize()
    assert bool(torch.isnan(tabs[5]).all()), 'stove_spn_bake wrote behind its tables'
    return [t.clone() for t in tabs[:5]]


@pytest.mark.parametrize('model,fill', A.BAKE_CASES)
def test_spn_bake_forward(model, fill):
    """all five tables per entry against RatSpn.tables() in float64: on the largest entry, entry-wise, and the softmax tables
    relatively down to 1e-30"""
    _, _, arena = A.bake_model(model, fill)
    plan, keep = _device_plan(arena)
    data = _dev(arena.data)
    got, again = _bake(data, plan), _bake(data, plan)
    ref, gaps = A.bake_reference(fill)['tables'], A.bake_gaps(fill)
    for name, g, g2, want in zip(A.TABLES, got, again, ref):
        assert not bool(torch.isnan(g).any()), name + ' holds entries the kernel did not write'
        assert _same_bits(g, g2), name
        key = 'arena.spn_bake.%s_%s.%s' % (model, fill, name)
        e, es = err(g, want), err_small(g, want)
        print('%s: %.3g / small %.3g (float32 gap %.3g / %.3g)' % (key, e, es, gaps['value'][name], gaps['value.small'][name]))
        check_ratio(key, e, A.bake_bar('value', gaps['value'][name]))
        check_ratio(key + '.small', es, A.bake_bar('value.small', gaps['value.small'][name]))
        if name in A.SOFTMAX_TABLES:
            er = A.rel_tiny(_np(g), want.numpy())
            print('%s.rel_tiny: %.3g (float32 gap %.3g)' % (key, er, gaps['value.rel_tiny'][name]))
            check_ratio(key + '.rel_tiny', er, A.bake_bar('value.rel_tiny', gaps['value.rel_tiny'][name]))
            assert float(g.min()) >= 0.0 and abs(float(g.double().sum()) - (120.0 if name == 'obj_wsum' else 1.0)) < 1e-4


def _group(name):
    spn = 'obj' if '.obj_spn.' in name else 'bg'
    if name.endswith('.means'):
        return spn + '.means'
    if name.endswith('.sigma_params'):
        return spn + '.sigma'
    layer = name.split('.vector_list.')[1].split('.')[0]                # layer 2 of the object SPN: its sum nodes; the last layer: the root
    return spn + ('.sums' if spn == 'obj' and layer == '2' else '.root')


def _bake_bwd(data, plan, ups, garena, calls):
    _lib, lib = _L()
    g = _lib.SpnTableGrads()
    g.obj_coef, g.obj_wsum, g.obj_wroot, g.bg_coef, g.bg_wroot = [u.data_ptr() for u in ups]
    out = []
    for _ in range(calls):
        _lib.check(lib.stove_spn_bake_bwd(data.data_ptr(), ctypes.byref(plan), ctypes.byref(g), garena.data_ptr(), _lib.stream()),
                   'stove_spn_bake_bwd')
        torch.cuda.synchronize()
        out.append(_np(garena).copy())
    return out


@pytest.mark.parametrize('model,fill', A.BAKE_CASES)
def test_spn_bake_backward(model, fill):
    """upstream table gradients from a seeded stream pushed into a pattern-filled gradient arena: the change per parameter tensor on
    three scales against autograd in float64; every float outside the SPN's tensors, the alignment pads included, bit-equal; a second
    call adds the same amount again; the whole thing twice, bit-equal"""
    _, _, arena = A.bake_model(model, fill)
    plan, keep = _device_plan(arena)
    data = _dev(arena.data)
    ups = [_dev(u) for u in A.bake_upstream(fill)]
    pat = A.bake_pattern(model, fill)
    first, second = _bake_bwd(data, plan, ups, _dev(pat), 2)
    again = _bake_bwd(data, plan, ups, _dev(pat), 1)[0]
    assert _same_bits(first, again)
    outside = A.outside_mask(model, fill)
    assert _same_bits(first[outside], pat[outside]) and _same_bits(second[outside], pat[outside])
    assert np.isfinite(first).all() and np.isfinite(second).all()
    ref, gaps = A.bake_reference(fill)['grads'], A.bake_gaps(fill)
    p64, f64, s64 = pat.astype(np.float64), first.astype(np.float64), second.astype(np.float64)
    for name, (o, k) in A.spn_spans(model, fill).items():
        want = ref[name].numpy()
        d1, d2 = f64[o:o + k] - p64[o:o + k], s64[o:o + k] - f64[o:o + k]
        key = 'arena.spn_bake_bwd.%s_%s.%s' % (model, fill, _group(name))
        for sfx, fn in (('', err), ('.l2', err_l2), ('.small', err_small)):
            check_ratio(key + sfx, fn(d1, want), A.bake_bar('grad' + sfx, gaps['grad' + sfx][name]))
        # three float32 roundings of sums no larger than (2 + PATTERN_SHIFT) max |d| lie between the two changes
        assert float(np.abs(d2 - d1).max()) <= 4e-7 * float(np.abs(d1).max()), name


def test_spn_tables_with_and_without_a_pending_prefetch():
    """ParamArena.spn_tables() after prefetch_images() (baked ahead on the second stream) and without: bit-equal, and the tables of
    the entry point called directly"""
    from stove_amd.arena import ParamArena
    from stove_amd.video_prediction.stove import Stove
    from gpu_helpers import fill_analytic
    st = fill_analytic(Stove(A.model_cfg(device=torch.device(DEV))), regime='init').to(DEV)
    arena = ParamArena(st, 1)
    assert arena.has_spn
    plain = arena.spn_tables()
    arena.prefetch_images()
    assert arena._pre is not None and 'spn' in arena._pre[0]
    ahead = arena.spn_tables()
    torch.cuda.synchronize()
    assert 'spn' not in arena._pre[0]                             # consumed
    for a, b in zip(plain[0][:3] + plain[1][:2] + plain[1][3:], ahead[0][:3] + ahead[1][:2] + ahead[1][3:]):
        assert a.data_ptr() != b.data_ptr() and _same_bits(a.reshape(-1), b.reshape(-1))
    direct = _bake(arena.data, arena._spn['plan'])
    for a, b in zip(plain[0][:3] + plain[1][:2], direct):
        assert _same_bits(a.reshape(-1), b)
    arena.drop_prefetched()


# ------------------------------------------------------------------------------------------------------------------ 2. gather / scatter
def _gather(data, src):
    _lib, lib = _L()
    n = int(src.size)
    out = torch.full((n + GUARD,), NAN, device=DEV)
    d, s = _dev(data), _dev(src if n else np.zeros(1, np.int32))
    _lib.check(lib.stove_arena_gather(d.data_ptr(), s.data_ptr(), out.data_ptr(), n, _lib.stream()), 'stove_arena_gather')
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[n:]).all())
    return _np(out[:n])


def _scatter(before, src, g):
    _lib, lib = _L()
    n = int(src.size)
    out = _dev(np.concatenate([before, np.full(GUARD, np.nan, np.float32)]))
    s, gg = _dev(src if n else np.zeros(1, np.int32)), _dev(g if n else np.zeros(1, np.float32))
    _lib.check(lib.stove_arena_scatter_add(gg.data_ptr(), s.data_ptr(), out.data_ptr(), n, _lib.stream()), 'stove_arena_scatter_add')
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[before.size:]).all())
    return _np(out[:before.size])


def _gather_scatter_exact(data, src, src_g, seed):
    want = A.gather_reference(data, src)
    got = _gather(data, src)
    assert _same_bits(got, want) and _same_bits(_gather(data, src), got)
    before, g = A.pattern(data.size, seed=seed), A.pattern(src_g.size, seed=seed + 1)
    want = A.scatter_reference(before, src_g, g)
    got = _scatter(before, src_g, g)
    assert _same_bits(got, want) and _same_bits(_scatter(before, src_g, g), got)
    untouched = np.ones(data.size, bool)
    untouched[src_g[src_g >= 0]] = False
    assert _same_bits(got[untouched], before[untouched])


@pytest.mark.parametrize('n', A.SYNTH_N)
def test_gather_and_scatter_at_the_block_edges(n):
    """n = 0, 1, 255, 256, 257 entries: the gather is numpy fancy indexing with zero where src < 0, the scatter np.add.at -- exactly"""
    gat, sca = A.synth_tables(n)
    _gather_scatter_exact(A.pattern(A.SYNTH_ARENA, seed=3), gat, sca, seed=n)


@pytest.mark.parametrize('cl,ac', A.GNN_CASES)
def test_gather_and_scatter_on_the_real_tables(cl, ac):
    """the index tables of cores 0 - 2 at cl = 16 / 32 / 64, with and without actions: the image the gather makes is the one
    Dynamics.param_image lays out without the arena, the scatter lands where np.add.at puts it"""
    from stove_amd import ops
    dyn, arena = A.gnn_case(cl, ac)
    data = arena.data.numpy()
    for k in range(3):
        src, src_g = (t.numpy() for t in arena._gnn[k])
        _gather_scatter_exact(data, src, src_g, seed=10 * cl + k)
        want = ops.gnn_width(cl).layout(*dyn.param_image(k)).detach().numpy()
        assert _same_bits(_gather(data, src), want)


# ------------------------------------------------------------------------------------------------------------------ 3. FlatAdam
def _adam(c, state, max_norm=None, sticky=False, hyper_dev=False, norm_out=True, ws=None, numel=None, null_ws=False):
    """stove_flat_adam on device copies of `state` (p, g, m, v, vmax or None, steps) -> dict of numpy arrays + rc.  hyper_dev: the
    constants come from device memory and the by-value arguments are NaN."""
    _lib, lib = _L()
    nseg = len(c['segs'])
    t = {k: (None if state[k] is None else _dev(np.asarray(state[k], np.float32))) for k in ('p', 'g', 'm', 'v', 'vmax', 'steps')}
    seg, tr = _dev(c['seg_of4']), _dev(c['trainable'])
    if ws is None:
        ws = torch.zeros(lib.stove_flat_adam_ws_bytes(nseg), dtype=torch.uint8, device=DEV)
    norm = torch.full((1 + GUARD,), NAN, device=DEV)
    hyper = A.HYPER + (float(max_norm) if max_norm is not None else 0.0,)
    hd = _dev(np.asarray(hyper, np.float32)) if hyper_dev else None
    by_value = (NAN,) * 5 if hyper_dev else hyper
    ptr = lambda x: None if x is None else x.data_ptr()           # noqa: E731
    rc = lib.stove_flat_adam(ptr(t['p']), ptr(t['g']), ptr(t['m']), ptr(t['v']), ptr(t['vmax']), c['numel'] if numel is None else numel,
                             seg.data_ptr(), tr.data_ptr(), t['steps'].data_ptr(), nseg, None if null_ws else ws.data_ptr(),
                             norm.data_ptr() if norm_out else None, ptr(hd), *by_value,
                             (1 if max_norm is not None else 0) | (2 if sticky else 0), _lib.stream())
    torch.cuda.synchronize()
    out = {k: (None if v is None else _np(v)) for k, v in t.items()}
    out.update(rc=rc, norm=float(norm[0]) if norm_out and rc == 0 else None, ws=ws, norm_buf=_np(norm))
    return out


def _adam_same(a, b):
    return all((a[k] is None and b[k] is None) or _same_bits(a[k], b[k]) for k in ('p', 'm', 'v', 'vmax', 'steps'))


def _untouched(got, c, active):
    """every float of p, m, v, vmax outside the segments that stepped -- the other segments and all pads -- and all of g: bit-equal"""
    keep = np.ones(c['numel'], bool)
    for (o, k, _), on in zip(c['segs'], active):
        if on:
            keep[o:o + k] = False
    assert keep.sum() > 0
    for key in ('p', 'm', 'v', 'vmax'):
        if c[key] is not None:
            assert _same_bits(got[key][keep], c[key][keep]), key
    assert _same_bits(got['g'], c['g'])


@pytest.mark.parametrize('case', A.ADAM_CASES, ids=A.adam_id)
def test_flat_adam_against_float64_adam(case):
    """one stove_flat_adam call on synthetic buffers against adam_reference in float64: both moments, AMSGrad's maximum, the norm and
    the step itself, per segment on its largest entry and entry-wise; step counts exactly; what does not step, and every pad, bit-equal"""
    size, clip, family, amsgrad = case
    c = A.adam_case(size, family, amsgrad)
    want, gaps = A.adam_expected(*case), A.adam_gaps(*case)
    mn = A.max_norm_of(c, clip)
    with_norm = (family == 'zero') != amsgrad                      # grad_norm_out given in half of the cases of every size and clip mode
    got = _adam(c, c, mn, norm_out=with_norm)
    assert got['rc'] == 0 and _adam_same(got, _adam(c, c, mn, norm_out=with_norm))
    assert not _np(got['ws'][1024:]).any()                         # the segment flags are cleared for the next call
    assert np.isnan(got['norm_buf'][1:]).all() and (with_norm or np.isnan(got['norm_buf'][0]))
    for k in ('p', 'm', 'v', 'vmax'):
        assert got[k] is None or np.isfinite(got[k]).all(), k
    assert np.array_equal(got['steps'].astype(np.float64), want['steps'])
    _untouched(got, c, want['active'])
    errors = A.adam_errors(got, want, c, c['segs'])
    assert set(errors) == set(gaps) - (set() if with_norm else {'norm'})
    for q, e in errors.items():
        print('arena.flat_adam.%s.%s: %.3g (float32 gap %.3g)' % (A.adam_id(case), q, e, gaps[q]))
        assert gaps[q] < 1e-4                                     # (asserted for every case on the CPU: no gap can make a bar meaningless)
        check_ratio('arena.flat_adam.%s.%s' % (size, q), e, A.adam_bar(gaps[q]))
    if clip == 'twice':                                            # the coefficient is exactly 1: the unclipped run, bit for bit
        assert _adam_same(got, _adam(c, c, None, norm_out=with_norm))


@pytest.mark.parametrize('size', list(A.ADAM_SIZES))
def test_flat_adam_reads_its_constants_from_device_memory(size):
    """hyper_dev given, the by-value constants NaN: bit-equal to the by-value run"""
    c = A.adam_case(size, 'unit', True)
    mn = A.max_norm_of(c, 'half')
    by_value, from_dev = _adam(c, c, mn), _adam(c, c, mn, hyper_dev=True)
    assert by_value['rc'] == 0 and from_dev['rc'] == 0 and _adam_same(by_value, from_dev)
    assert _bits(np.float32(by_value['norm'])) == _bits(np.float32(from_dev['norm']))
    assert not _same_bits(by_value['p'], c['p'])


def test_flat_adam_strict_zero_gradient_bit_over_two_calls():
    """a gradient, then zeros, at a multi-block size with one workspace: with bit 2 of `clip` the segments that stepped step again on
    their momentum (two reference steps in float64); without it the second call changes nothing"""
    c = A.adam_case(A.STRICT_ZERO_SIZE, 'unit', True)
    zeros = dict(c, g=np.zeros_like(c['g']))
    for sticky in (False, True):
        first = _adam(c, c, sticky=sticky)
        second = _adam(zeros, dict(first, g=zeros['g']), sticky=sticky, ws=first['ws'])
        assert first['rc'] == 0 and second['rc'] == 0
        r1, want = A.adam_two_calls(sticky)
        assert np.array_equal(first['steps'].astype(np.float64), r1['steps'])
        assert np.array_equal(second['steps'].astype(np.float64), want['steps'])
        flags = _np(second['ws'][1024:]).view(np.int32)
        assert np.array_equal(flags != 0, want['flags'])
        if not sticky:
            assert _adam_same(first, second) and not flags.any()
            continue
        assert want['active'].tolist() == r1['active'].tolist() and np.array_equal(want['steps'], c['steps'] + 2.0 * r1['active'])
        _untouched(dict(second, g=c['g']), c, want['active'])
        gaps = A.adam_two_calls_gaps()
        for q, e in A.adam_errors(dict(second, norm=None), want, c, c['segs'], calls=2).items():
            print('arena.flat_adam.strict_zero.%s: %.3g (float32 gap %.3g)' % (q, e, gaps[q]))
            assert gaps[q] < 1e-4
            check_ratio('arena.flat_adam.strict_zero.' + q, e, A.adam_bar(gaps[q]))


def test_flat_adam_refusals_leave_the_buffers_alone():
    """a numel that is no multiple of 4 and a null workspace are refused, nothing written"""
    c = A.adam_case('n1028', 'unit', True)
    for kw in (dict(numel=c['numel'] - 2), dict(null_ws=True)):
        got = _adam(c, c, A.max_norm_of(c, 'half'), **kw)
        assert got['rc'] == INVALID
        for k in ('p', 'g', 'm', 'v', 'vmax', 'steps'):
            assert _same_bits(got[k], c[k]), k
        assert np.isnan(got['norm_buf']).all() and not _np(got['ws']).any()


# ------------------------------------------------------------------------------------------------------------------ 4. bw_transform
def _bw(x, N=None, C=None, P=None):
    _lib, lib = _L()
    n, c, p = x.shape
    out = torch.full((n * p + GUARD,), NAN, device=DEV)
    xd = _dev(x)
    fn = lib.stove_bw_transform_u8 if x.dtype == torch.uint8 else lib.stove_bw_transform
    rc = fn(xd.data_ptr(), out.data_ptr(), n if N is None else N, c if C is None else C, p if P is None else P, _lib.stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[n * p:]).all())
    return rc, out[:n * p].view(n, p).cpu()


@pytest.mark.parametrize('u8', [False, True], ids=['f32', 'u8'])
@pytest.mark.parametrize('C,P,N', A.BW_SHAPES)
def test_bw_transform_is_the_clamped_channel_sum_bit_for_bit(C, P, N, u8):
    """clamp(sum over channels in channel order, 0, 1) in float32 (u8: of float32(x_c) / 255) -- bit-equal to torch on the CPU, on frames
    where the clamp acts on both sides; u8 also within 1.2e-7 of the float64 value"""
    x = A.bw_inputs(C, P, N, u8)
    want = A.bw_reference(x)
    rc, got = _bw(x)
    assert rc == 0 and not bool(torch.isnan(got).any())
    assert _same_bits(got, want), (C, P, N, u8, float((got - want).abs().max()))
    assert _same_bits(_bw(x)[1], got)
    if u8:
        e = float((got.double() - A.bw_sums(x).clamp(0.0, 1.0)).abs().max())
        check('arena.bw_transform_u8.c%d.float64' % C, e, 1.2e-7)


@pytest.mark.parametrize('u8', [False, True], ids=['f32', 'u8'])
def test_bw_transform_refusals(u8):
    """a pixel count that is no multiple of 4 and channels = 0 are refused, the output untouched; zero frames return with nothing written"""
    x = A.bw_inputs(3, 1024, 1, u8)
    for kw in (dict(P=1022), dict(C=0)):
        rc, out = _bw(x, **kw)
        assert rc == INVALID and bool(torch.isnan(out).all())
    rc, out = _bw(x, N=0)
    assert rc == 0 and bool(torch.isnan(out).all())


# ------------------------------------------------------------------------------------------------------------------ 5. noise
def _signed(v):
    return v - 2 ** 64 if v >= 2 ** 63 else v


def _noise(seed, call, n, offset=0):
    _lib, lib = _L()
    state = torch.tensor([_signed(seed), _signed(call)], dtype=torch.int64, device=DEV)
    out = torch.full((offset + n + A.NOISE_GUARD,), NAN, device=DEV)
    rc = lib.stove_noise_normal(out.data_ptr() + 4 * offset, n, state.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    return rc, _np(out), [int(v) % 2 ** 64 for v in state.cpu().tolist()]


@pytest.mark.parametrize('state', list(A.NOISE_STATES))
@pytest.mark.parametrize('n', A.NOISE_N)
def test_noise_is_philox_4x32_10_and_box_muller(n, state):
    """stove_noise_normal with the state written directly against the numpy reference: Philox-4x32-10 at counter (call, thread), key
    (seed), u = ((r >> 8) + 0.5) / 2^24, two Box-Muller pairs per thread; the guard floats behind n stay NaN, state[1] advances by one
    (2^64 - 1 wraps to 0), state[0] stays"""
    seed, call = A.NOISE_STATES[state]
    rc, out, after = _noise(seed, call, n)
    assert rc == 0 and after == [seed, (call + 1) % 2 ** 64]
    assert np.isnan(out[n:]).all(), 'the tail path wrote past n'
    got, want = out[:n], A.noise_reference(seed, call, n)
    assert np.isfinite(got).all() and _same_bits(_noise(seed, call, n)[1][:n], got)
    e = float((np.abs(got.astype(np.float64) - want) / np.maximum(1.0, np.abs(want))).max())
    print('arena.noise.%s.n%d: %.3g' % (state, n, e))
    check('arena.noise.%s' % state, e, A.noise_bar())
    check('arena.noise.measured', e, A.noise_bar())
    assert A.noise_bar() <= A.NOISE_CAP


def test_noise_refuses_a_misaligned_output():
    rc, out, after = _noise(3, 4, 16, offset=1)
    assert rc == INVALID and np.isnan(out).all() and after == [3, 4]
