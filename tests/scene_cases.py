"""The cases, float64 / float32 references, float32 gaps and bars of the scene-likelihood tests at every object count
(tests/test_scene_cases_cpu.py checks the conditions stated here from the oracle alone, tests/test_gpu_scene_counts.py holds the three
fused pipelines to them).  Nothing here touches a GPU.

Cases (CASES): the counts no test compared directly with O.scene_likelihood -- the first count of every rung of the nmax_of (3 / 6 / 8)
and nmax_ch (3 / 8) ladders, one object, every occluder slot in use, four channels -- on the any-geometry, colour and 32 x 32
pipelines, each under the 'analytic', 'init' and 'stress' weights.  DEGENERATE: exact ties in the occlusion chain, an object wholly
outside the frame and objects at both scale bounds, at 4, 7 and 8 objects on each pipeline.  All inputs are float32 values; the
float64 run, the float32 run and the device see the same numbers.

Underflow rule: a parameter tensor whose float64 gradient has its largest entry below UNDERFLOW = 1e-30 cannot be held relatively in
float32 (the oracle's own float32 run is 40 % .. 100 % off on them); the device's gradient of it must be finite and below 1e-30 too.
Conditions: at most 4 such tensors per (case, regime), all under sup.bg_spn.vector_list.0., in at most 3 of the 39 pairs (met by:
any_50x50_n1 / analytic, ch_32_c4_n3 / analytic, mono_n7 / stress).  Under the saturated 'stress' weights the 32 x 32 cases
drive the leaf gradients of one or two background replicas below float64's range as well: exactly zero in the float64 oracle (at
nearly every seed; the filter max |g| > 0 of the existing tests drops them).  Those have no scale at all; they are kept apart from
the underflowing ones (classify), lie under the same prefix, and the device's gradient of them must be finite and below 1e-30.

Bars: gpu_helpers.regime_bar(base, gap) -- the base bars of the existing scene tests (log p and its parts 6e-6; dz 3e-4 / 3e-4 / 5e-3;
parameter gradients 3e-4 / 3.5e-4 / 1.5e-2 for err / err_l2 / err_small) or 6 x the oracle's own float32-to-float64 distance `gap` for
that quantity on that (case, regime) under the same error function, whichever is larger.  So that a large gap cannot hide a failure
every gap is capped (CAPS; a case whose gap exceeds its cap is reseeded, the cap stays):
  err gaps 2e-3 (largest measured 1.28e-3: a background leaf tensor, ch_32_c3_n1 / stress), log p gaps 1e-6 (largest measured 2.6e-7);
  err_l2 and err_small gaps at twice the largest measured over the 39 pairs and the 9 degenerate cases (printed by
  tests/test_scene_cases_cpu.py):
    dz    err_l2 4.14e-4   err_small 1.24e-3
    grad  err_l2 6.75e-4   err_small 6.94e-3
  the three parts of log p, which the issue did not measure: largest err gap 7.6e-7, capped at twice that.
"""
import functools

import torch

import stove_oracle as O
from gpu_helpers import err, err_l2, err_small, regime_bar
from helpers import oracle_setup

REGIMES = ('analytic', 'init', 'stress')
UNDERFLOW = 1e-30
UNDERFLOW_PREFIX = 'sup.bg_spn.vector_list.0.'
MAX_UNDERFLOWING_TENSORS, MAX_UNDERFLOWING_PAIRS = 4, 3

# id: (pipeline, W, H, channels, objects, align_corners); frames are (.., channels, W, H), the last dimension is grid_sample's x
CASES = {
    'any_50x50_n1': ('any', 50, 50, 1, 1, False),
    'any_28x40_n2': ('any', 28, 40, 1, 2, True),
    'any_28x40_n4': ('any', 28, 40, 1, 4, True),
    'any_40x28_n7': ('any', 40, 28, 1, 7, False),
    'ch_32_c3_n1': ('colour', 32, 32, 3, 1, False),
    'ch_32_c3_n4': ('colour', 32, 32, 3, 4, False),
    'ch_32_c3_n7': ('colour', 32, 32, 3, 7, True),
    'ch_24x20_c4_n8': ('colour', 24, 20, 4, 8, False),
    'ch_32_c4_n3': ('colour', 32, 32, 4, 3, False),
    'mono_n4': ('mono', 32, 32, 1, 4, False),
    'mono_n5': ('mono', 32, 32, 1, 5, False),
    'mono_n7': ('mono', 32, 32, 1, 7, False),
    'mono_n8': ('mono', 32, 32, 1, 8, False),
}
# id: what is added to the case's seed (a case that broke a condition is reseeded, never the condition).  With the seeds of
# test_scene_likelihood_vs_oracle_ragged (11 + objects), mono_n4 / analytic, mono_n5 / stress and mono_n8 / stress each had four
# underflowing tensors: six pairs in all, where three are allowed.  The first shift at which the case has none in any regime:
SEED_SHIFT = {'mono_n4': 1, 'mono_n5': 5, 'mono_n8': 2}
ORDER_CASES = ('any_40x28_n7', 'ch_32_c3_n7', 'mono_n7')

# degenerate geometry: the first count of each rung and the full rung, on each pipeline, 'analytic' weights, 6 frames
DEGENERATE = {'deg_%s_n%d' % (p, n): (p,) + g + (n, False)
              for p, g in (('any', (40, 28, 1)), ('colour', (32, 32, 3)), ('mono', (32, 32, 1))) for n in (4, 7, 8)}
ALL = {**CASES, **DEGENERATE}

BASE = {'log_p': 6e-6, 'part': 6e-6,
        'dz': 3e-4, 'dz.l2': 3e-4, 'dz.small': 5e-3,
        'grad': 3e-4, 'grad.l2': 3.5e-4, 'grad.small': 1.5e-2}
ERR_FN = {'': err, '.l2': err_l2, '.small': err_small}
MEASURED = {'dz.l2': 4.14e-4, 'dz.small': 1.24e-3, 'grad.l2': 6.75e-4, 'grad.small': 6.94e-3, 'part': 7.6e-7}     # largest gaps, docstring
CAPS = {'log_p': 1e-6, 'dz': 2e-3, 'grad': 2e-3}


def pairs():
    return [(case, regime) for case in CASES for regime in REGIMES]


def degenerate_pairs():
    return [(case, 'analytic') for case in DEGENERATE]


def oracle_cfg(case):
    pipeline, W, H, C, n_obj, ac = ALL[case]
    cfg = dict(num_obj=n_obj, width=W, height=H, align_corners=ac)
    if pipeline == 'colour':
        cfg.update(channels=C, debug_bw=False)
    if n_obj != 3:
        cfg['debug_match_objects'] = 'greedy'
    return cfg


def _f32(t):
    return t.float().double()


@functools.lru_cache(maxsize=None)
def inputs(case):
    """-> (x, z, w, view): clips x (n, T, C, W, H), z (frames * objects, 4) = [sx, sy, x, y] and per-frame weights w, float32 values
    in float64; view: the scored frames are x[:, 1:], handed over as that view (else all of x).  Shared: read-only."""
    pipeline, W, H, C, n_obj, ac = ALL[case]
    shift = SEED_SHIFT.get(case, 0)
    if case in DEGENERATE:
        return _degenerate_inputs(case, shift)
    if pipeline == 'mono':
        # test_gpu_spn.test_scene_likelihood_vs_oracle_ragged: 45 frames (no multiple of the 64-glimpse tile), every object of
        # frame 0 on top of the first
        g = torch.Generator().manual_seed(11 + n_obj + shift)
        nb, t = 5, 9
        r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)          # noqa: E731
        x = r(nb, t, 1, 32, 32) ** 2
        z = torch.zeros(nb * t, n_obj, 4, dtype=torch.float64)
        z[..., 0] = 0.1 + 0.6 * r(nb * t, n_obj)
        z[..., 1] = z[..., 0] * (0.75 + 0.5 * r(nb * t, n_obj))
        z[..., 2:] = 1.9 * r(nb * t, n_obj, 2) - 0.95
        z[0, :, 2:] = z[0, 0:1, 2:]
        return _f32(x), _f32(z.flatten(0, 1)), _f32(torch.linspace(0.5, 1.5, nb * t, dtype=torch.float64)), False
    # test_gpu_colour._inputs: 3 clips of 4 scored frames, scales 0.12 .. 0.42, centres in +-0.95 (some glimpses hang over the edge)
    n, T = 3, 4
    gen = torch.Generator().manual_seed(1000 + 7 * W + H + 31 * C + n_obj + shift)
    x = torch.rand(n, T + 1, C, W, H, generator=gen)
    z = torch.empty(n * T * n_obj, 4)
    z[:, 0] = 0.12 + 0.3 * torch.rand(z.shape[0], generator=gen)
    z[:, 1] = z[:, 0] * (0.8 + 0.4 * torch.rand(z.shape[0], generator=gen))
    z[:, 2:] = 1.9 * torch.rand(z.shape[0], 2, generator=gen) - 0.95
    wgt = torch.randn(n * T, generator=gen)
    return x.double(), z.double(), wgt.double(), True


def _degenerate_inputs(case, shift):
    """2 clips of 3 scored frames.  Frame 0: every object at one centre and scale (exact ties in the occlusion chain); frame 1: object
    2 wholly outside the frame (centre 1.5, scale 0.15); frame 2: object 0 at max_obj_scale, object 3 at min_obj_scale; 3 .. 5 random."""
    pipeline, W, H, C, n_obj, ac = ALL[case]
    c = O.default_config()
    n, T = 2, 3
    gen = torch.Generator().manual_seed(5000 + 100 * list(DEGENERATE).index(case) + shift)
    x = torch.rand(n, T + 1, C, W, H, generator=gen)
    if pipeline == 'mono':
        x = x ** 2
    z = torch.empty(n * T, n_obj, 4)
    z[..., 0] = 0.12 + 0.3 * torch.rand(n * T, n_obj, generator=gen)
    z[..., 1] = z[..., 0] * (0.8 + 0.4 * torch.rand(n * T, n_obj, generator=gen))
    z[..., 2:] = 1.9 * torch.rand(n * T, n_obj, 2, generator=gen) - 0.95
    z[0] = z[0, 0:1].clone()
    z[1, 2] = torch.tensor([0.15, 0.15, 1.5, 1.5])
    z[2, 0, :2] = c.max_obj_scale
    z[2, 3, :2] = c.min_obj_scale
    wgt = torch.randn(n * T, generator=gen)
    return x.double(), z.flatten(0, 1).double(), wgt.double(), True


def scored(x, view):
    return x[:, 1:] if view else x


def swap_first_two(z, n_obj):
    """z with objects 0 and 1 of every frame exchanged (occlusion depends on the order)"""
    z = z.view(-1, n_obj, 4).clone()
    z[:, [0, 1]] = z[:, [1, 0]]
    return z.flatten(0, 1)


def _setup(case, regime, dtype):
    cfg, structs, params = oracle_setup(dtype, regime=regime, **oracle_cfg(case))
    return cfg, structs, {k: v for k, v in params.items() if k.startswith('sup.') and not k.startswith('sup.encoder.')}


@functools.lru_cache(maxsize=None)
def reference(case, regime, dtype=torch.float64):
    """O.scene_likelihood(parts=True) + the backward under the case's frame weights, in `dtype` on the float32 roundings of the case's
    inputs -> dict(log_p (frames,), parts (frames, 3) = bg / patch / overlap, dz, grads {reference name: gradient}).  Once per
    (case, regime, dtype), shared: read-only."""
    cfg, structs, params = _setup(case, regime, dtype)
    x, z, w, view = inputs(case)
    zz = z.to(dtype).clone().requires_grad_()                 # a fresh leaf after the cast
    lp, bg, pl, ov = O.scene_likelihood(cfg, params, structs, scored(x, view).to(dtype), zz, parts=True)
    (lp * w.to(dtype)).sum().backward()
    return {'log_p': lp.detach(), 'parts': torch.stack([bg, pl, ov], -1).detach(), 'dz': zz.grad,
            'grads': {k: v.grad for k, v in params.items() if v.grad is not None}}


def swapped_log_p(case, regime):
    """the float64 oracle's log p with objects 0 and 1 of every frame exchanged"""
    cfg, structs, params = _setup(case, regime, torch.float64)
    x, z, w, view = inputs(case)
    with torch.no_grad():
        return O.scene_likelihood(cfg, params, structs, scored(x, view), swap_first_two(z, ALL[case][4]))


def classify(case, regime):
    """-> (compared, underflowing, zero): the names of the parameter gradients that are held relatively, that underflow float32
    (largest float64 entry below UNDERFLOW) and that the float64 oracle leaves exactly zero"""
    compared, under, zero = [], [], []
    for k, g in reference(case, regime)['grads'].items():
        m = float(g.abs().max())
        (zero if m == 0.0 else under if m < UNDERFLOW else compared).append(k)
    return compared, under, zero


@functools.lru_cache(maxsize=None)
def gaps(case, regime):
    """The oracle's float32-to-float64 distance per quantity under the error function it is checked with: {'log_p', 'part.bg' /
    '.patch' / '.overlap', 'dz', 'dz.l2', 'dz.small', 'grad' / 'grad.l2' / 'grad.small': {name: gap}}.  Never from a kernel."""
    hi, lo = reference(case, regime), reference(case, regime, torch.float32)
    out = {'log_p': err(lo['log_p'], hi['log_p'])}
    for i, k in enumerate(('bg', 'patch', 'overlap')):
        out['part.' + k] = err(lo['parts'][:, i], hi['parts'][:, i])
    compared = classify(case, regime)[0]
    for sfx, fn in ERR_FN.items():
        out['dz' + sfx] = fn(lo['dz'], hi['dz'])
        out['grad' + sfx] = {k: fn(lo['grads'][k], hi['grads'][k]) for k in compared}
    return out


def cap(key):
    """the largest gap a (case, regime) may have for the quantity `key` ('log_p', 'part', 'dz', 'dz.l2', 'grad.small', ...)"""
    return CAPS[key] if key in CAPS else 2.0 * MEASURED[key]


def bar(key, gap):
    """the tolerance of quantity `key` at the oracle's float32 gap `gap` (asserted to lie within its cap)"""
    assert gap <= cap(key), (key, gap, cap(key))
    return regime_bar(BASE[key], gap)
