"""The three fused scene-likelihood pipelines -- 32 x 32 one channel (stove_scene_fwd / _bwd), run-time geometry (stove_scene_fwd_any /
_bwd_any), colour (stove_scene_fwd_ch / _bwd_ch) -- against the float64 oracle at the object counts no test compared directly: the
first count of every rung of the nmax_of / nmax_ch ladders, one object, every occluder slot in use, four channels; under the
'analytic', 'init' and the saturated 'stress' weights.  Cases, references, gaps, bars and the underflow rule: tests/scene_cases.py
(its conditions are checked from the oracle alone by tests/test_scene_cases_cpu.py).

a. every (case, regime) through Supair.likelihood: log p, its three parts per frame, dz and every parameter gradient; a second run bit
   for bit.  b. the same frames with objects 0 and 1 exchanged on the device alone must MISS the log p bar: the bars see a wrong
   occluder slot.  c. exact ties in the occlusion chain, an object outside the frame, objects at both scale bounds.  d. the C entry
   points on `saved` / `ws` buffers of exactly the queried sizes between guard bands.

Every achieved error is printed next to the oracle's own float32 gap and the bar (pytest -s, or the captured output of a failure)."""
import ctypes

import pytest
import torch

import scene_cases as S
from gpu_helpers import check_ratio, err, fill_analytic

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


def _supair(case, regime):
    from stove_amd.video_prediction.supair import Supair
    sup = Supair(_cfg(**S.oracle_cfg(case)))
    pipeline = S.ALL[case][0]
    assert sup.obj_spn._kind == ('obj_any' if pipeline == 'colour' else 'obj') and sup.bg_spn._kind == 'bg'
    sup = fill_analytic(sup, 'sup.', regime=regime).to(DEV)
    sup.step_counter = 0
    return sup


class _Watch:
    """Wraps the autograd entry of the pipeline a case must take and keeps what it returned (log p and the per-frame parts)."""

    def __init__(self, pipeline):
        from stove_amd import ops
        self.pipeline, self.out = pipeline, []
        self.fn = ops._SceneChFn if pipeline == 'colour' else ops._SceneFn

    def __enter__(self):
        self.orig = self.fn.apply

        def apply(*a):
            if self.pipeline != 'colour':
                assert (a[-1] is None) == (self.pipeline == 'mono'), 'geometry %s on the %s pipeline' % (a[-1], self.pipeline)
            self.out.append(self.orig(*a))
            return self.out[-1]
        self.fn.apply = apply
        return self

    def __exit__(self, *exc):
        self.fn.apply = self.orig


def _run(sup, case, z):
    """-> (log p, parts (frames, 3), dz) of Supair.likelihood + backward under the case's weights on the device"""
    pipeline = S.ALL[case][0]
    x, _, w, view = S.inputs(case)
    xs = S.scored(x.float().to(DEV), view)
    zd = z.float().to(DEV).requires_grad_()
    with _Watch(pipeline) as watch:
        lp, _ = sup.likelihood(xs, zd)
    assert len(watch.out) == 1, 'the fused %s pipeline was not taken' % pipeline
    (lp * w.float().to(DEV)).sum().backward()
    return lp.detach(), watch.out[0][1].detach(), zd.grad.clone()


def _report(key, what, e, gap, bar):
    print(f'scene_counts.{key} {what}: {e:.3g} (oracle f32 gap {gap:.3g}, bar {bar:.3g})')
    check_ratio('scene_counts.' + key, e, bar)


def _compare(case, regime):
    pipeline = S.ALL[case][0]
    ref, gaps = S.reference(case, regime), S.gaps(case, regime)
    compared, under, zero = S.classify(case, regime)
    sup = _supair(case, regime)
    z = S.inputs(case)[1]
    lp, parts, dz = _run(sup, case, z)
    what = f'{case}/{regime}'
    assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(dz).all())
    _report(pipeline + '.log_p', what, err(lp, ref['log_p']), gaps['log_p'], S.bar('log_p', gaps['log_p']))
    for i, k in enumerate(('bg', 'patch', 'overlap')):
        _report(pipeline + '.part_' + k, what, err(parts[:, i], ref['parts'][:, i]), gaps['part.' + k], S.bar('part', gaps['part.' + k]))
    for sfx, fn in S.ERR_FN.items():
        _report(pipeline + '.dz' + sfx, what, fn(dz, ref['dz']), gaps['dz' + sfx], S.bar('dz' + sfx, gaps['dz' + sfx]))
    got = {'sup.' + k: p.grad for k, p in sup.named_parameters()}
    for sfx, fn in S.ERR_FN.items():
        rows = []
        for k in compared:
            assert got[k] is not None and bool(torch.isfinite(got[k]).all()), k
            gap = gaps['grad' + sfx][k]
            rows.append((fn(got[k], ref['grads'][k]), gap, S.bar('grad' + sfx, gap), k))
        e, gap, bar, k = max(rows, key=lambda r: r[0] / r[2])
        print(f'scene_counts.{pipeline}.grad{sfx} {what} worst of {len(rows)}, {k}: {e:.3g} (oracle f32 gap {gap:.3g}, bar {bar:.3g})')
        for e, gap, bar, k in rows:
            check_ratio(f'scene_counts.{pipeline}.grad{sfx}', e, bar)
    assert len(compared) >= 6
    for k in under + zero:           # no scale in float32 (scene_cases: underflow rule): finite and as small
        assert bool(torch.isfinite(got[k]).all()) and float(got[k].abs().max()) < S.UNDERFLOW, (k, float(got[k].abs().max()))
    sup.zero_grad()
    lp2, _, dz2 = _run(sup, case, z)
    assert torch.equal(lp, lp2) and torch.equal(dz, dz2)


@pytest.mark.parametrize('case,regime', S.pairs(), ids=lambda v: v)
def test_scene_pipelines_against_the_oracle_at_the_uncovered_counts(case, regime):
    _compare(case, regime)


@pytest.mark.parametrize('case', S.ORDER_CASES)
def test_the_log_p_bar_sees_two_objects_in_the_wrong_order(case):
    """The device gets objects 0 and 1 of every frame exchanged, the oracle does not: log p must then miss its bar (the oracle itself
    moves by more than 100 x the bar under the exchange, tests/test_scene_cases_cpu.py)."""
    pipeline, n_obj = S.ALL[case][0], S.ALL[case][4]
    ref, gap = S.reference(case, 'analytic')['log_p'], S.gaps(case, 'analytic')['log_p']
    lp, _, _ = _run(_supair(case, 'analytic'), case, S.swap_first_two(S.inputs(case)[1], n_obj))
    e, bar = err(lp, ref), S.bar('log_p', gap)
    print(f'scene_counts.{pipeline}.swapped_log_p {case}: {e:.3g} (bar {bar:.3g}, {e / bar:.3g} x)')
    assert e > bar, (e, bar)


@pytest.mark.parametrize('case,regime', S.degenerate_pairs(), ids=lambda v: v)
def test_scene_pipelines_on_degenerate_geometry(case, regime):
    _compare(case, regime)


# ------------------------------------------------------------------------------------------------ d. workspace and saved-activation sizes
GUARD = 1024                       # floats: 4 KiB in front of and behind every buffer
PATTERN = 0x7FC5A5A5               # a NaN of its own: a value read from a guard or from unwritten workspace poisons what it reaches
SIZE_GEOMETRY = {'mono': (32, 32, 1, False), 'any': (40, 28, 1, False), 'colour': (32, 32, 3, False)}
_TABLES = {}


def _guarded(n_floats):
    """`n_floats` floats carved out of a larger allocation filled with PATTERN (control_harness.guarded does this for given tensors;
    here the buffer is scratch, and the bits are compared, not the values) -> (pointer, view, whole buffer)"""
    buf = torch.full((n_floats + 2 * GUARD,), PATTERN, dtype=torch.int32, device=DEV)
    return ctypes.c_void_p(buf.data_ptr() + 4 * GUARD), buf[GUARD:GUARD + n_floats].view(torch.float32), buf


def _intact(buf):
    return bool((buf[:GUARD] == PATTERN).all()) and bool((buf[-GUARD:] == PATTERN).all())


def _tables(pipeline):
    """the baked tables of the pipeline's SPNs under the 'analytic' weights (they do not depend on the object count), detached"""
    if pipeline not in _TABLES:
        from stove_amd.video_prediction.supair import Supair
        W, H, C, ac = SIZE_GEOMETRY[pipeline]
        kw = dict(width=W, height=H, align_corners=ac)
        if pipeline == 'colour':
            kw.update(channels=C, debug_bw=False)
        sup = fill_analytic(Supair(_cfg(**kw)), 'sup.').to(DEV)
        with torch.no_grad():
            _TABLES[pipeline] = (sup.obj_spn.tables(), sup.bg_spn.tables(), float(sup.c.overlap_beta), sup.c.patch_width, sup.c.patch_height)
    return _TABLES[pipeline]


@pytest.mark.parametrize('n_obj', [1, 3, 4, 6, 7, 8])
@pytest.mark.parametrize('pipeline', list(SIZE_GEOMETRY))
def test_saved_and_workspace_fit_their_size_queries(pipeline, n_obj):
    """The C entry points called as stove_amd/ops.py calls them, with `saved` and `ws` of exactly stove_scene_*_floats / *_bytes (ops
    allocates one float more): the guard bands around them, and around ll, parts and dz, stay untouched, and ll and dz are the ops
    path's bit for bit.  Nothing is read or written out of bounds on purpose: the guards lie inside one allocation."""
    from stove_amd import _lib, ops
    from stove_amd._lib import SpnTableGrads, check, ptr, stream
    lib = _lib.load()
    W, H, C, ac = SIZE_GEOMETRY[pipeline]
    obj_tabs, bg_tabs, beta, pw, ph = _tables(pipeline)
    nf = 5
    gen = torch.Generator().manual_seed(7000 + 10 * list(SIZE_GEOMETRY).index(pipeline) + n_obj)
    frames = torch.rand(nf, C * W * H, generator=gen).to(DEV)
    z = torch.empty(nf * n_obj, 4)
    z[:, 0] = 0.12 + 0.3 * torch.rand(z.shape[0], generator=gen)
    z[:, 1] = z[:, 0] * (0.8 + 0.4 * torch.rand(z.shape[0], generator=gen))
    z[:, 2:] = 1.9 * torch.rand(z.shape[0], 2, generator=gen) - 0.95
    z = z.to(DEV)
    dll = torch.randn(nf, generator=gen).to(DEV)

    zo = z.clone().requires_grad_()
    if pipeline == 'colour':
        ll_o, _ = ops.scene_likelihood_colour(frames, zo, obj_tabs, bg_tabs, n_obj, beta, (C, W, H, pw, ph, ac))
    else:
        ll_o, _ = ops.scene_likelihood(frames, zo, obj_tabs, bg_tabs, n_obj, beta, None, None if pipeline == 'mono' else (W, H, ac))
    (ll_o * dll).sum().backward()

    bufs = {}

    def carve(name, n_floats):
        p, view, bufs[name] = _guarded(int(n_floats))
        return p, view

    ll_p, ll = carve('ll', nf)
    parts_p, _ = carve('parts', nf * 3)
    dz_p, dz = carve('dz', nf * n_obj * 4)
    bc, bw, bs = bg_tabs[:3]
    st = torch.cuda.current_stream(DEV).cuda_stream
    if pipeline == 'colour':
        oc, ow, orr, lscope, slot, shape = obj_tabs
        R, G, S_, D, lmax = (int(v) for v in shape)
        grads = [torch.empty_like(t) for t in (oc, ow, orr, bc, bw)]
        saved_p, _ = carve('saved', lib.stove_scene_saved_floats_ch(nf, n_obj, C, W, H, R, G, S_, D, lmax, 1))
        ws_p, _ = carve('ws', (lib.stove_scene_bwd_ws_bytes_ch(nf, n_obj, C, W, H, R, G, S_, D, lmax) + 3) // 4)
        head = (ptr(lscope), ptr(slot), ptr(oc), ptr(ow), ptr(orr), R, G, S_, D, lmax, ptr(bs), ptr(bc), ptr(bw), bc.numel(),
                frames.data_ptr(), ptr(z), nf, n_obj, 0, 0, C, W, H, pw, ph, int(ac), beta)
        check(lib.stove_scene_fwd_ch(*head, ll_p, parts_p, saved_p, stream(), 1), 'stove_scene_fwd_ch')
        check(lib.stove_scene_bwd_ch(*head, saved_p, ptr(dll), dz_p, *[ptr(g) for g in grads], ws_p, stream(), None), 'stove_scene_bwd_ch')
    else:
        oc, ow, orr, osc, ols = obj_tabs
        grads = [torch.empty_like(t) for t in (oc, ow, orr, bc, bw)]
        g = SpnTableGrads()
        g.obj_coef, g.obj_wsum, g.obj_wroot, g.bg_coef, g.bg_wroot = [ptr(t) for t in grads]
        t = ops._tables(obj=(osc, ols, oc, ow, orr), bg=(bs, bc, bw))
        head = (ctypes.byref(t), frames.data_ptr(), ptr(z), nf, n_obj, 0, 0)
        if pipeline == 'any':
            saved_p, _ = carve('saved', lib.stove_scene_saved_floats_any(nf, n_obj, W * H, 1))
            ws_p, _ = carve('ws', (lib.stove_scene_bwd_ws_bytes_any(nf, n_obj, W * H) + 3) // 4)
            check(lib.stove_scene_fwd_any(*head, W, H, int(ac), beta, ll_p, parts_p, saved_p, stream(), 1), 'stove_scene_fwd_any')
            check(lib.stove_scene_bwd_any(*head, W, H, int(ac), beta, saved_p, ptr(dll), dz_p, ctypes.byref(g), ws_p, st, None),
                  'stove_scene_bwd_any')
        else:
            assert lib.stove_scene_fwd_floats(nf, n_obj, 1) == lib.stove_scene_saved_floats(nf, n_obj)
            saved_p, _ = carve('saved', lib.stove_scene_saved_floats(nf, n_obj))
            ws_p, _ = carve('ws', (lib.stove_scene_bwd_ws_bytes(nf, n_obj) + 3) // 4)
            check(lib.stove_scene_fwd_from(*head, beta, ll_p, parts_p, saved_p, stream(), None, 1), 'stove_scene_fwd_from')
            check(lib.stove_scene_bwd(*head, beta, saved_p, ptr(dll), dz_p, ctypes.byref(g), ws_p, stream()), 'stove_scene_bwd')
    torch.cuda.synchronize()
    for name, buf in bufs.items():
        assert _intact(buf), 'the guard bands of `%s` were written (%s, %d objects)' % (name, pipeline, n_obj)
    assert torch.equal(ll, ll_o.detach()), float((ll - ll_o.detach()).abs().max())
    assert torch.equal(dz.view(-1, 4), zo.grad), float((dz.view(-1, 4) - zo.grad).abs().max())
