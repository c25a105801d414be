"""The cases, float64 references, float32 gaps and bars of the kernels that open and close a training step (csrc/arena.hip and
noise_normal_k of csrc/state.hip): the SPN table bake and its backward, the arena gather / scatter, FlatAdam's three kernels, both
bw_transform kernels and the noise generator.  tests/test_arena_cases_cpu.py pins the references and asserts the conditions stated here
without a GPU, tests/test_gpu_arena_kernels.py holds the kernels to them through the C entry points.  Nothing here touches a GPU.

1. Table bake.  BAKE_CASES = ('supair' | 'stove') x ('analytic' | 'init' | 'stress' | 'edges').  The models are built in float32 on the
   CPU, filled by the rule of the regime and bound to a ParamArena there; the arena's buffer and index plan are what the device gets.
   'edges' = 'analytic' plus plant_edges.  The reference (bake_reference) is RatSpn.tables() and autograd on a float64 Supair holding
   the same float32 values; its float32 run gives the gaps.  Upstream table gradients: bake_upstream, a seeded normal stream.
   Errors: err on the largest entry, err_small entry-wise, and for the three softmax tables rel_tiny: the largest relative error over
   the entries above TINY = 1e-30, because err_small's floor of 1e-3 of the largest weight says nothing about a weight of 4e-19 either.
   Bars: 1e-6 values / 1e-5 gradients, or 6 x the reference's own float32 gap under the same error function on the same case
   (gpu_helpers.regime_bar), every gap capped at twice the largest measured on the CPU (BAKE_MEASURED; test_arena_cases_cpu prints them).
   rel_tiny's bar by the same rule: float32 rounds p - max to 2^-24 of up to 180, which exp turns into 5e-6 relative, in torch as in
   the kernel; the float64 run has no such rounding.
2. Gather / scatter.  Exact.  SYNTH_N synthetic tables and the real tables of cores 0 - 2 at GNN_CASES.
3. FlatAdam.  adam_reference: one step of torch's single-tensor Adam / AMSGrad with clip_grad_norm_ folded in, per-segment step
   counts, in numpy at a given dtype.  ADAM_CASES: size x clip x family x amsgrad (adam_case builds the buffers; adam_segments lays
   the five KINDS of segment out, the synthetic sizes ending in a 'last' one).  Errors (adam_errors): per segment that steps, on its
   largest entry (seg_err) and entry-wise with a floor of 1e-3 of it (seg_small) -- the gradient scales span 18 decades, a norm over
   the whole buffer would see the 1e6 segments only.  Bars: 1e-6, or 6 x the same errors of the reference's own float32 run (adam_gaps).
4. bw_transform.  BW_SHAPES; bw_inputs draws frames on which the clamp acts on both sides; bw_reference is float32 torch on the CPU.
5. Noise.  philox4x32_10 and noise_reference in numpy; the bar is 4 x the error measured on the device, at most 1e-4 (noise_bar).
"""
import functools

import numpy as np
import torch

from gpu_helpers import err, err_l2, err_small, fill_analytic, regime_bar

TINY = 1e-30

# ------------------------------------------------------------------------------------------------------------------ 1. table bake
BAKE_MODELS = ('supair', 'stove')
BAKE_FILLS = ('analytic', 'init', 'stress', 'edges')
BAKE_CASES = [(m, f) for m in BAKE_MODELS for f in BAKE_FILLS]
TABLES = ('obj_coef', 'obj_wsum', 'obj_wroot', 'bg_coef', 'bg_wroot')
TABLE_FLOATS = (18000, 12000, 600, 55296, 108)
SOFTMAX_TABLES = ('obj_wsum', 'obj_wroot', 'bg_wroot')
BAKE_BASE = {'value': 1e-6, 'value.small': 1e-6, 'value.rel_tiny': 1e-6, 'grad': 1e-5, 'grad.l2': 1e-5, 'grad.small': 1e-5}
# the largest float32 gaps of the reference over the four fills (printed by tests/test_arena_cases_cpu.py); a gap may be twice that
# (all six under 'stress': the object SPN's root column for the values, its leaves' sigma_params -- s (1 - s) at |rho| = 8 -- for the gradients)
BAKE_MEASURED = {'value': 5.46e-7, 'value.small': 5.45e-7, 'value.rel_tiny': 2.46e-6, 'grad': 1.11e-5, 'grad.l2': 9.73e-6, 'grad.small': 4.28e-5}
PATTERN_SHIFT = 2.0 ** -9               # the pattern under an SPN tensor's gradient, in units of the gradient's largest entry


def model_cfg(dtype=torch.float32, **kw):
    from stove_amd.video_prediction.config import StoveConfig
    cfg = StoveConfig()
    cfg.num_obj, cfg.width, cfg.height, cfg.random_seed = 3, 32, 32, 42
    cfg.device, cfg.dtype = torch.device('cpu'), dtype
    cfg.action_conditioned, cfg.action_space = False, None
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def plant_edges(sup):
    """On top of the 'analytic' fill: sigma_params of +-30 and +-100 in leaves of both SPNs (expf overflows to inf, the variance lies
    exactly at a bound, s (1 - s) = 0), a sum column of all-equal entries, a sum column with one entry 90 above the rest, both root
    columns scaled by 20."""
    obj, bg = sup.obj_spn, sup.bg_spn
    with torch.no_grad():
        for spn, which in ((obj, (0, 7, 23)), (bg, (1, 4))):
            for li in which:
                rho = list(spn.vector_list[0])[li].sigma_params.view(-1)
                for j, v in enumerate((30.0, -30.0, 100.0, -100.0)):
                    rho[3 * li + j::41] = v
        sums = list(obj.vector_list[2])
        sums[0].params[:, 0] = 0.25
        sums[5].params[:, 9] = 0.25
        col = sums[1].params[:, 3]
        col[17] = col.max() + 90.0
        col = sums[11].params[:, 0]
        col[99] = col.max() + 90.0
        obj.output_vector.params.mul_(20.0)
        bg.output_vector.params.mul_(20.0)
    return sup


def _fill(module, prefix, fill):
    fill_analytic(module, prefix, 'analytic' if fill == 'edges' else fill)
    if fill == 'edges':
        plant_edges(module if hasattr(module, 'obj_spn') else module.sup)
    return module


@functools.lru_cache(maxsize=None)
def bake_model(model, fill):
    """-> (module, sup, arena): a float32 CPU Supair ('supair') or Stove ('stove'), filled, bound to a ParamArena.  Shared: read-only."""
    from stove_amd.arena import ParamArena
    from stove_amd.video_prediction.stove import Stove
    from stove_amd.video_prediction.supair import Supair
    if model == 'supair':
        module = _fill(Supair(model_cfg()), 'sup.', fill)
        sup = module
    else:
        module = _fill(Stove(model_cfg()), '', fill)
        sup = module.sup
    return module, sup, ParamArena(module, world_size=1)


def spn_names(module):
    """{canonical name ('sup.obj_spn. ...'): parameter} of the 74 SPN tensors of a Supair or a Stove"""
    pre = '' if hasattr(module, 'sup') else 'sup.'
    out = {}
    for n, p in module.named_parameters():
        n = pre + n
        if n.startswith(('sup.obj_spn.', 'sup.bg_spn.')):
            out[n] = p
    return out


def spn_spans(model, fill):
    """{canonical name: (float offset in the arena, numel)} of the SPN tensors"""
    module, _, arena = bake_model(model, fill)
    return {n: (arena.offset[id(p)], p.numel()) for n, p in spn_names(module).items()}


def tables_of(sup):
    """the five float tables of a Supair, in the order of TABLES"""
    oc, ow, orr = sup.obj_spn.tables()[:3]
    bc, bw = sup.bg_spn.tables()[:2]
    return [oc, ow, orr, bc, bw]


@functools.lru_cache(maxsize=None)
def bake_upstream(fill):
    """upstream gradients of the five tables: standard normal draws, float32 values"""
    g = torch.Generator().manual_seed(7100 + BAKE_FILLS.index(fill))
    return [torch.randn(n, generator=g, dtype=torch.float64).float() for n in TABLE_FLOATS]


@functools.lru_cache(maxsize=None)
def bake_reference(fill, dtype=torch.float64):
    """RatSpn.tables() and autograd in `dtype` on a CPU Supair that holds the float32 values of the case ->
    dict(tables [5 flat tensors], grads {canonical name: gradient}).  The tables of a Supair do not depend on what surrounds it, so
    one reference serves both models (test_arena_cases_cpu asserts that).  Shared: read-only."""
    from stove_amd.video_prediction.supair import Supair
    src = bake_model('supair', fill)[1]
    sup = Supair(model_cfg(dtype)).to(dtype)
    sup.load_state_dict({k: v.detach().to(dtype) for k, v in src.state_dict().items()})
    tabs = tables_of(sup)
    loss = sum((t.reshape(-1) * u.to(dtype)).sum() for t, u in zip(tabs, bake_upstream(fill)))
    loss.backward()
    grads = {n: p.grad.detach().reshape(-1) for n, p in spn_names(sup).items() if p.grad is not None}
    return {'tables': [t.detach().reshape(-1) for t in tabs], 'grads': grads}


def rel_tiny(a, b):
    """the largest |a - b| / |b| over the entries with |b| > TINY"""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    ok = np.abs(b) > TINY
    return float((np.abs(a - b)[ok] / np.abs(b)[ok]).max()) if ok.any() else 0.0


def _np(t):
    return t.detach().double().cpu().numpy() if torch.is_tensor(t) else np.asarray(t, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def bake_gaps(fill):
    """the reference's float32-to-float64 distance: {'value' / 'value.small' / 'value.rel_tiny': {table: gap},
    'grad' / 'grad.l2' / 'grad.small': {name: gap}}.  Never from a kernel."""
    hi, lo = bake_reference(fill), bake_reference(fill, torch.float32)
    out = {k: {} for k in BAKE_BASE}
    for name, a, b in zip(TABLES, lo['tables'], hi['tables']):
        out['value'][name], out['value.small'][name] = err(a, b), err_small(a, b)
        if name in SOFTMAX_TABLES:
            out['value.rel_tiny'][name] = rel_tiny(_np(a), _np(b))
    for n, b in hi['grads'].items():
        a = lo['grads'][n]
        out['grad'][n], out['grad.l2'][n], out['grad.small'][n] = err(a, b), err_l2(a, b), err_small(a, b)
    return out


def bake_bar(key, gap):
    """the tolerance of quantity `key` at the reference's float32 gap `gap` (asserted to lie within its cap)"""
    assert gap <= 2.0 * BAKE_MEASURED[key], (key, gap, 2.0 * BAKE_MEASURED[key])
    return regime_bar(BAKE_BASE[key], gap)


def bake_pattern(model, fill):
    """what grad_arena holds before the backward: sin(i) + 2 (never zero) outside the SPN tensors, the pads included; under an SPN
    tensor +-PATTERN_SHIFT x the largest entry of its reference gradient -- small against the gradient, so that `after - before`
    keeps the gradient's small entries (a pattern of O(1) would leave them 6e-8 of absolute rounding), and far above the bars, so
    that an overwrite instead of an accumulation is 2e-3 off"""
    _, _, arena = bake_model(model, fill)
    pat = (np.sin(np.arange(arena.numel, dtype=np.float64)) + 2.0).astype(np.float32)
    ref = bake_reference(fill)['grads']
    for n, (o, k) in spn_spans(model, fill).items():
        scale = float(ref[n].abs().max()) * PATTERN_SHIFT
        pat[o:o + k] = (scale * np.where(np.arange(k) % 2 == 0, 1.0, -1.0)).astype(np.float32)
    return pat


def outside_mask(model, fill):
    """True at every arena float that belongs to no SPN tensor (other parameters and the alignment pads)"""
    _, _, arena = bake_model(model, fill)
    m = np.ones(arena.numel, dtype=bool)
    for o, k in spn_spans(model, fill).values():
        m[o:o + k] = False
    return m


# ------------------------------------------------------------------------------------------------------------------ 2. gather / scatter
SYNTH_N = (0, 1, 255, 256, 257)
SYNTH_ARENA = 300
GNN_CASES = [(cl, ac) for cl in (16, 32, 64) for ac in (False, True)]


def synth_tables(n):
    """-> (gather table, scatter table) of n entries into an arena of SYNTH_ARENA floats: the gather table repeats addresses and
    holds -1 in a seventh of its entries, the scatter table names every address at most once"""
    rs = np.random.RandomState(900 + n)
    gat = rs.randint(0, SYNTH_ARENA, size=n).astype(np.int32)
    sca = rs.permutation(SYNTH_ARENA)[:n].astype(np.int32)
    gat[np.arange(n) % 7 == 3] = -1
    sca[np.arange(n) % 7 == 5] = -1
    return gat, sca


@functools.lru_cache(maxsize=None)
def gnn_case(cl, ac):
    """-> (dyn, arena): a float32 CPU Dynamics at state-code length cl, with or without actions, 'analytic' weights, bound to an arena"""
    from stove_amd.arena import ParamArena
    from stove_amd.video_prediction.dynamics import Dynamics
    kw = dict(cl=cl, transition_lik_std=[0.01] * (cl // 2))
    if ac:
        kw.update(action_conditioned=True, action_space=9, debug_core_appearance=True)
    dyn = fill_analytic(Dynamics(model_cfg(**kw)), 'dyn.')
    return dyn, ParamArena(dyn, world_size=1)


def gather_reference(data, src):
    data, src = np.asarray(data), np.asarray(src)
    out = np.zeros(src.shape, dtype=data.dtype)
    ok = src >= 0
    out[ok] = data[src[ok]]
    return out


def scatter_reference(before, src, g):
    out, src, g = np.array(before, copy=True), np.asarray(src), np.asarray(g)
    ok = src >= 0
    np.add.at(out, src[ok], g[ok])
    return out


def pattern(n, seed=0):
    """n float32 values in [1, 3], none zero"""
    return (np.sin(np.arange(n, dtype=np.float64) * 0.7 + seed) + 2.0).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ 3. FlatAdam
KINDS = ('train', 'train_zero', 'frozen', 'frozen_zero', 'last')
STEPS_IN = (0.0, 1.0, 9.0, 1000.0, 100000.0)
GRAD_SCALES = (1.0, 1e-12, 1e6)
ADAM_SIZES = {'n4': 4, 'n1024': 1024, 'n1028': 1028, 'n262144': 262144, 'n262148': 262148, 'stove': None}
CLIPS = ('off', 'half', 'twice')
FAMILIES = ('zero', 'unit')
ADAM_CASES = [(s, c, f, a) for s in ADAM_SIZES for c in CLIPS for f in FAMILIES for a in (True, False)]
HYPER = tuple(float(np.float32(x)) for x in (1e-3, 0.9, 0.999, 1e-8))          # lr, beta1, beta2, eps as the float32 values the kernel gets
ADAM_BASE = 1e-6
SCAN_SPAN = 256 * 256 * 4                 # floats one trip of grad_scan_k's grid covers
# fractions of the buffer the synthetic segments end at (no multiple of 4 anywhere: every segment has pads)
_CUTS = (0.03, 0.11, 0.19, 0.26, 0.38, 0.47, 0.55, 0.68, 0.77, 0.9, 1.0)


@functools.lru_cache(maxsize=None)
def stove_segment_sizes():
    from stove_amd.video_prediction.stove import Stove
    return tuple(p.numel() for p in Stove(model_cfg()).parameters())


def adam_segments(size):
    """-> list of (offset, numel, kind) with offsets on float4 boundaries, and the padded total"""
    numel = ADAM_SIZES[size]
    if size == 'stove':
        sizes = list(stove_segment_sizes())
    elif numel == 4:
        sizes = [1]
    else:
        ends, sizes, prev = [], [], 0
        for c in _CUTS[:-1]:
            e = int(numel * c) // 4 * 4
            ends.append(e)
        ends.append(numel)
        for i, e in enumerate(ends):
            sizes.append(e - prev - (1 + i % 3))            # 1 .. 3 pad floats behind every segment
            prev = e
    segs, off = [], 0
    for i, k in enumerate(sizes):
        # the synthetic layouts end in a 'last' segment: at 262 148 floats its only gradient lies in the one float4 of the scan's second trip
        kind = KINDS[(i + 4) % 5] if len(sizes) > 1 else 'last'
        if kind == 'last' and k % 4 == 0:
            kind = 'train'                                   # 'last' needs pad floats in the segment's final float4
        segs.append((off, k, kind))
        off += (k + 3) // 4 * 4
    assert numel is None or off == numel, (size, off, numel)
    return segs, off


@functools.lru_cache(maxsize=None)
def adam_case(size, family, amsgrad):
    """The buffers of a case, float32 numpy, shared: read-only.  p: zeros ('zero') or sin-shaped O(1) values ('unit'), pads 7;
    g: scale x normal draws by the segment's kind, pads 0; m, v: non-zero, scaled with the segment's gradients, pads 0; vmax:
    v x 2 at even entries, v / 2 at odd ones, pads 3; steps: STEPS_IN by segment."""
    segs, numel = adam_segments(size)
    rs = np.random.RandomState(4000 + list(ADAM_SIZES).index(size))
    p = np.full(numel, 7.0, np.float32)
    g, m, v = (np.zeros(numel, np.float32) for _ in range(3))
    vmax = np.full(numel, 3.0, np.float32)
    seg_of4 = np.zeros(numel // 4, np.int32)
    trainable = np.zeros(len(segs), np.uint8)
    steps = np.zeros(len(segs), np.float32)
    stepping = 0
    for i, (o, k, kind) in enumerate(segs):
        a = stepping if kind in ('train', 'last') else i                # the segments that step walk through every scale and count
        stepping += kind in ('train', 'last')
        scale = GRAD_SCALES[a % 3]
        seg_of4[o // 4:(o + k + 3) // 4] = i
        trainable[i] = kind in ('train', 'train_zero', 'last')
        steps[i] = STEPS_IN[a % 5] if len(segs) > 1 else 9.0
        draw = rs.standard_normal(k)
        if kind in ('train', 'frozen'):
            g[o:o + k] = scale * draw
        elif kind == 'last':
            g[o + k - 1] = scale * (1.0 + abs(draw[-1]))
        m[o:o + k] = scale * 0.5 * rs.standard_normal(k)
        v[o:o + k] = (scale * (0.5 + rs.random_sample(k))) ** 2
        vmax[o:o + k] = v[o:o + k] * np.where(np.arange(k) % 2 == 0, 2.0, 0.5)
        p[o:o + k] = 0.0 if family == 'zero' else np.sin(0.37 * np.arange(k) + i) + 0.25 * np.sign(np.sin(0.37 * np.arange(k) + i) + 1e-9)
    return {'p': p, 'g': g, 'm': m, 'v': v, 'vmax': vmax if amsgrad else None, 'seg_of4': seg_of4, 'trainable': trainable,
            'steps': steps, 'segs': segs, 'numel': numel}


def grad_norm64(g):
    return float(np.sqrt((np.asarray(g, np.float64) ** 2).sum()))


def max_norm_of(case_buffers, clip):
    """None ('off'), half the float64 norm ('half'), twice it ('twice': the coefficient is exactly 1) -- as the float32 the kernel gets"""
    if clip == 'off':
        return None
    return float(np.float32(grad_norm64(case_buffers['g']) * (0.5 if clip == 'half' else 2.0)))


def adam_reference(p, g, m, v, vmax, segs, trainable, steps, hyper, max_norm=None, dtype=np.float64, flags=None, sticky=False):
    """One step of torch.optim.Adam (single-tensor path, weight_decay 0; AMSGrad when vmax is given) behind clip_grad_norm_, restated:
        norm = ||g||_2 over every gradient;  g' = g min(1, max_norm / (norm + 1e-6))
        per tensor that is trainable and has a non-zero gradient entry (or kept its flag, `sticky`), with t = its step count + 1:
        m += (1 - b1) (g' - m);  v = b2 v + (1 - b2) g'^2;  vmax = max(vmax, v)
        p -= lr / (1 - b1^t) m / (sqrt(vmax or v) / sqrt(1 - b2^t) + eps);  step count = t
    every other tensor is left alone.  All arithmetic in `dtype` (the bias corrections in float64 either way, like torch's host side).
    -> dict(p, m, v, vmax, steps, norm, flags, active)"""
    f = dtype
    lr, b1, b2, eps = (f(x) for x in hyper)
    p, g, m, v = (np.array(x, dtype=f) for x in (p, g, m, v))
    vmax = None if vmax is None else np.array(vmax, dtype=f)
    steps = np.array(steps, dtype=np.float64)
    flags = np.zeros(len(segs), bool) if flags is None else np.array(flags, dtype=bool)
    norm = np.sqrt((g * g).sum(dtype=f))
    coef = f(1.0) if max_norm is None else min(f(1.0), f(max_norm) / (norm + f(1e-6)))
    active = np.zeros(len(segs), bool)
    one = f(1.0)
    for i, (o, k, _) in enumerate(segs):
        hi = o + (k + 3) // 4 * 4                           # the kernel sees the pads of a segment as part of it
        flags[i] |= bool((g[o:hi] != 0).any())
        if not (trainable[i] and flags[i]):
            continue
        active[i] = True
        t = steps[i] + 1.0
        bc1, sqrt_bc2 = f(1.0 - float(b1) ** t), f(np.sqrt(1.0 - float(b2) ** t))
        gg = g[o:hi] * coef
        m[o:hi] = m[o:hi] + (one - b1) * (gg - m[o:hi])
        v[o:hi] = b2 * v[o:hi] + (one - b2) * gg * gg
        x = v[o:hi]
        if vmax is not None:
            vmax[o:hi] = np.maximum(vmax[o:hi], v[o:hi])
            x = vmax[o:hi]
        p[o:hi] = p[o:hi] - (lr / bc1) * m[o:hi] / (np.sqrt(x) / sqrt_bc2 + eps)
        steps[i] = t
    if not sticky:
        flags[:] = False
    return {'p': p, 'm': m, 'v': v, 'vmax': vmax, 'steps': steps, 'norm': float(norm), 'flags': flags, 'active': active}


@functools.lru_cache(maxsize=None)
def adam_expected(size, clip, family, amsgrad, dtype=np.float64):
    """adam_reference on the buffers of the case.  Shared: read-only."""
    c = adam_case(size, family, amsgrad)
    return adam_reference(c['p'], c['g'], c['m'], c['v'], c['vmax'], c['segs'], c['trainable'], c['steps'], HYPER,
                          max_norm_of(c, clip), dtype)


def seg_err(a, b, segs, active):
    """the largest, over the active segments, of max |a - b| / max |b| within the segment"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    worst = 0.0
    for (o, k, _), on in zip(segs, active):
        if on:
            worst = max(worst, float(np.abs(a[o:o + k] - b[o:o + k]).max() / (np.abs(b[o:o + k]).max() + 1e-300)))
    return worst


def seg_small(a, b, segs, active, slack=None):
    """entry-wise: the largest, over the entries of the active segments, of (|a - b| - slack) / (|b| + 1e-3 max_segment |b|); `slack`
    (per entry) is what the comparison forgives before it counts, e.g. half an ulp of the parameter the step was added to"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    worst = 0.0
    for (o, k, _), on in zip(segs, active):
        if on:
            d = np.abs(a[o:o + k] - b[o:o + k])
            if slack is not None:
                d = np.maximum(d - slack[o:o + k], 0.0)
            worst = max(worst, float((d / (np.abs(b[o:o + k]) + 1e-3 * np.abs(b[o:o + k]).max() + 1e-300)).max()))
    return worst


def adam_errors(got, want, before, segs, calls=1):
    """{quantity: error} of a result (dict of arrays: p, m, v, vmax or None, norm or None) against adam_reference's `want`, `before`
    the buffers of the case.  'step': p_after - p_before against the reference's, forgiving half a float32 ulp of p per call (each
    call rounds p once)."""
    act = want['active']
    out = {}
    for k in ('m', 'v', 'vmax'):
        if want[k] is not None and got.get(k) is not None:
            out[k], out[k + '.small'] = seg_err(got[k], want[k], segs, act), seg_small(got[k], want[k], segs, act)
    p0 = np.asarray(before['p'], np.float64)
    step_got, step_want = np.asarray(got['p'], np.float64) - p0, np.asarray(want['p'], np.float64) - p0
    half_ulp = 0.5 * calls * np.spacing(np.maximum(np.abs(np.asarray(before['p'], np.float32)), np.abs(np.asarray(got['p'], np.float32)))).astype(np.float64)
    half_ulp[p0 == 0.0] = 0.0                       # from zero, p is the rounded step itself: nothing to forgive
    out['step'] = seg_err(np.sign(step_got - step_want) * np.maximum(np.abs(step_got - step_want) - half_ulp, 0.0) + step_want, step_want, segs, act)
    out['step.small'] = seg_small(step_got, step_want, segs, act, slack=half_ulp)
    if got.get('norm') is not None:
        out['norm'] = abs(got['norm'] - want['norm']) / want['norm']
    return out


@functools.lru_cache(maxsize=None)
def adam_gaps(size, clip, family, amsgrad):
    """adam_errors of the numpy reference's own float32 run against its float64 run.  Never from a kernel."""
    c = adam_case(size, family, amsgrad)
    lo, hi = adam_expected(size, clip, family, amsgrad, np.float32), adam_expected(size, clip, family, amsgrad)
    return adam_errors(lo, hi, c, c['segs'])


STRICT_ZERO_SIZE = 'n262148'


@functools.lru_cache(maxsize=None)
def adam_two_calls(sticky, dtype=np.float64):
    """a gradient, then zeros, on the 'unit' AMSGrad buffers of STRICT_ZERO_SIZE -> (first result, second result).  Shared: read-only."""
    c = adam_case(STRICT_ZERO_SIZE, 'unit', True)
    a = adam_reference(c['p'], c['g'], c['m'], c['v'], c['vmax'], c['segs'], c['trainable'], c['steps'], HYPER, None, dtype, None, sticky)
    b = adam_reference(a['p'], np.zeros_like(c['g']), a['m'], a['v'], a['vmax'], c['segs'], c['trainable'], a['steps'], HYPER, None, dtype,
                       a['flags'], sticky)
    return a, b


def adam_two_calls_gaps():
    c = adam_case(STRICT_ZERO_SIZE, 'unit', True)
    return adam_errors(dict(adam_two_calls(True, np.float32)[1], norm=None), adam_two_calls(True)[1], c, c['segs'], calls=2)


def adam_bar(gap):
    return regime_bar(ADAM_BASE, gap)


def adam_id(case):
    size, clip, family, amsgrad = case
    return '%s-%s-%s-%s' % (size, clip, family, 'ams' if amsgrad else 'adam')


# ------------------------------------------------------------------------------------------------------------------ 4. bw_transform
BW_SHAPES = [(C, P, N) for C in (1, 3, 6) for P in (4, 1024, 2500, 28 * 40) for N in (1, 37)]
# (C, P, N, u8): what is added to the seed.  A shape on which the float32 reference itself lies further than 1.2e-7 from the float64
# value (six roundings of x / 255 and five of the sum can reach 1.6e-7 just below 1) is reseeded; the bound stays.  First seed that holds:
BW_SEED_SHIFT = {(6, 2500, 37, True): 2}


@functools.lru_cache(maxsize=None)
def bw_inputs(C, P, N, u8=False):
    """(N, C, P) frames whose channel sums spread over [-0.4, 1.6] (float) / [0, 1.6] (u8; one channel: [0, 1]): a per-pixel level
    split over the channels by random positive shares, plus planted pixels in every run of 16 -- level 1.5; every channel 0; one
    channel 1 (255), the rest 0; level -0.3 (float); two channels 0.5 each (float, C >= 2).  Shared: read-only."""
    rs = np.random.RandomState(6000 + 100 * C + P % 97 + N + (50 if u8 else 0) + BW_SEED_SHIFT.get((C, P, N, u8), 0))
    level = rs.uniform(0.0 if u8 else -0.4, 1.6, size=(N, 1, P))
    share = rs.random_sample((N, C, P)) + 0.1
    share /= share.sum(1, keepdims=True)
    x = level * share
    i = np.arange(N * P).reshape(N, 1, P)
    j, ch = i % 16, np.arange(C).reshape(1, C, 1)
    x = np.where(j == 0, 1.5 * share, x)                                    # the first four pixels of a 4-pixel frame: above 1,
    x = np.where(j == 1, 0.0, x)                                            # exactly 0,
    x = np.where(j == 2, np.where(ch == (i // 16) % C, 1.0, 0.0), x)        # exactly 1,
    if not u8:
        x = np.where(j == 3, -0.3 * share, x)                               # below 0
        if C >= 2:
            x = np.where(j == 7, np.where(ch < 2, 0.5, 0.0), x)
    if u8:
        return torch.from_numpy(np.clip(np.round(x * 255.0), 0, 255).astype(np.uint8))
    return torch.from_numpy(x.astype(np.float32))


def bw_sums(x):
    """the unclamped channel sums in float64 (u8: of x / 255)"""
    x = x.double() / 255.0 if x.dtype == torch.uint8 else x.double()
    return x.sum(1)


def bw_reference(x):
    """clamp(sum over channels in channel order, 0, 1) in float32 torch on the CPU; u8: of float32(x_c) / 255"""
    x = x.float() / 255.0 if x.dtype == torch.uint8 else x
    s = x[:, 0].clone()
    for c in range(1, x.shape[1]):
        s = s + x[:, c]
    return s.clamp(0.0, 1.0)


# ------------------------------------------------------------------------------------------------------------------ 5. noise
NOISE_N = (1, 3, 4, 5, 1023, 1024, 1025, 262147)
NOISE_STATES = {'zero': (0, 0), 'seed_max': (2 ** 64 - 1, 5), 'call_hi': (0x0123456789ABCDEF, 2 ** 32), 'call_max': (77, 2 ** 64 - 1)}
NOISE_GUARD = 8
NOISE_CAP = 1e-4
# the largest |got - ref| / max(1, |ref|) measured on an MI355X over NOISE_N x NOISE_STATES (profiles/arena_parity.json, key
# arena.noise.measured: 1.5246e-5, state 'seed_max'); the bar is 4 x that, at most NOISE_CAP.  None: not measured, the cap alone holds.
NOISE_MEASURED = 1.525e-5
PHILOX_KAT = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)
_M32 = np.uint64(0xffffffff)


def philox4x32_10(counter, key):
    """Philox-4x32-10 (Salmon et al., SC'11): counter = 4 arrays, key = 2 arrays of 32-bit words held in uint64 -> 4 arrays"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _M32 for c in counter)
    k0, k1 = (np.asarray(k, dtype=np.uint64) & _M32 for k in key)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def noise_bar():
    return NOISE_CAP if NOISE_MEASURED is None else min(4.0 * NOISE_MEASURED, NOISE_CAP)


@functools.lru_cache(maxsize=None)
def noise_reference(seed, call, n):
    """the n draws of state (seed, call) in float64: thread i makes elements 4 i .. 4 i + 3 from Philox at counter
    (call lo, call hi, i lo, i hi), key (seed lo, seed hi); u = ((r >> 8) + 0.5) / 2^24; Box-Muller on (c0, c1) and on (c2, c3)"""
    i = np.arange((n + 3) // 4, dtype=np.uint64)
    full = lambda v: np.full(i.shape, v, dtype=np.uint64)          # noqa: E731
    c = philox4x32_10((full(call & 0xffffffff), full(call >> 32), i & _M32, i >> np.uint64(32)),
                      (full(seed & 0xffffffff), full(seed >> 32)))
    u = [((w >> np.uint64(8)).astype(np.float64) + 0.5) / 16777216.0 for w in c]
    r0, r1 = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
    a0, a1 = 2.0 * np.pi * u[1], 2.0 * np.pi * u[3]
    return np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], 1).reshape(-1)[:n]
