"""Cases, inputs and float64 references of the planning kernels at every object and action count: what tests/test_plan_cases_cpu.py
checks on the CPU and tests/test_gpu_plan_counts.py holds the kernels to (stove_reward_head_fwd / _bwd, csrc/reward_head.hip;
stove_plan_expand, csrc/plan.hip; stove_plan_search, csrc/plan_tree.hip).

Weight fills: 'analytic' and 'init' of tests/golden/analytic_weights.py, and 'spread' -- the 'init' fill with the weight tensors of the
five reward-head layers (not their biases) times a factor k per case, applied to the float64 values before anything is rounded,
so that the oracle's parameter dict and the module hold the same numbers.  Under the committed fills the reward hardly moves (0.5267 ..
0.5319 over a whole case); under 'spread' it covers a tenth of (0, 1) and more, and a wrong weight element or a dropped object shows.

Inputs of the expansion cases are a committed fixture (tests/golden/plan_counts_inputs.npz, written by tools/make_plan_inputs.py):
every ReLU pre-activation of the reward head has to keep 1e-4 of its layer's largest away from zero, and a case holds up to 5e5 of
them, so no seed of a whole case meets that; make_inputs() redraws single trees (until the A first steps are clear) and then the random
actions of single rows (until the row's L further steps are); the L = 70 case, whose late steps set the layers' largest, is drawn
by make_inputs_long, a tree with its rows at a time.  The reward-head cases redraw single items as they are built."""
import collections
import functools
import os

import numpy as np
import torch

import stove_oracle as O
from analytic_weights import analytic_tensor, fan_ins

GAMMA = 0.95
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FIXTURE = os.path.join(GOLDEN, 'plan_counts_inputs.npz')
RH_LAYERS = ('dyn.reward_head0.0', 'dyn.reward_head0.2', 'dyn.reward_head1.0', 'dyn.reward_head1.2', 'dyn.reward_head1.4')
RH_PACKED = tuple(n + s for n in RH_LAYERS for s in ('.weight', '.bias'))        # the order of the kernels' parameter block
RELU_MARGIN = 1e-4                    # |pre-activation| / the layer's largest, float64
REGIMES = ('analytic', 'init', 'spread')
# k of the 'spread' fill: per expansion case (SPREAD_K, by case name), per search case (by search_id) and per object count for the
# reward-head cases (RH_SPREAD_K), chosen on the CPU; tests/test_plan_cases_cpu.py asserts the three conditions on every one of them.
# (One k per (N, app_dim) does not exist: the cases of one (N, app_dim) differ in action count and nonlinearity, and e.g. at
# (5, 3) the nine-action ELU case saturates at a k where the one-action case has not begun to spread.)
SPREAD_K = {
    'counts-N1-A9-app3-M3-L5-elu': 2.75,
    'counts-N2-A9-app3-M3-L5-lrelu': 2.6875,
    'counts-N3-A9-app3-M3-L5-elu': 2.125,
    'counts-N4-A9-app3-M3-L5-lrelu': 2.25,
    'counts-N5-A9-app3-M3-L5-elu': 1.875,
    'counts-N6-A9-app3-M3-L5-elu': 1.6875,
    'counts-N6-A9-app3-M3-L5-lrelu': 2.0625,
    'counts-N7-A9-app3-M3-L5-lrelu': 2.0625,
    'counts-N8-A9-app3-M3-L5-lrelu': 1.8125,
    'few-N2-A1-app3-M3-L5-elu': 2.375,
    'few-N2-A2-app3-M3-L5-lrelu': 2.6875,
    'few-N5-A1-app3-M3-L5-lrelu': 2.25,
    'few-N5-A2-app3-M3-L5-elu': 1.875,
    'limit-N2-A64-app3-M17-L2-lrelu': 2.75,
    'limit-N4-A64-app12-M2-L5-elu': 1.9375,
    'limit-N5-A64-app3-M17-L2-lrelu': 2.1875,
    'long-N2-A2-app0-M2-L70-lrelu': 2.0625,
    'noapp-N1-A9-app0-M3-L5-elu': 2.625,
    'noapp-N4-A9-app0-M3-L5-lrelu': 2.25,
    'noapp-N7-A9-app0-M3-L5-elu': 1.5625,
    'onestep-N3-A9-app3-M3-L1-lrelu': 2.5625,
    'rows-N3-A9-app3-M114-L2-lrelu': 2.4375,
    'wide-N3-A9-app12-M3-L5-elu': 2.125,
    'wide-N8-A9-app12-M3-L5-elu': 1.5625,
}
SEARCH_SPREAD_K = {'N1-A1-M2-D2-R6': 3.375, 'N2-A64-M3-D2-R8': 2.625, 'N6-A2-M70-D4-R16': 1.9375, 'N8-A9-M3-D5-R12': 1.8125}
RH_SPREAD_K = {1: 2.0625, 2: 1.875, 3: 1.8125, 4: 1.75, 5: 1.75, 6: 1.6875, 7: 1.6875, 8: 1.625}
RH_SATURATED_K = 3.0


# ------------------------------------------------------------------------------------------------ configurations and parameters
def plan_cfg(N, A, app_dim, elu=False):
    """the model behind an expansion: action-conditioned, A actions, app_dim appearance columns in the core (0: none)"""
    cfg = dict(num_obj=N, action_conditioned=True, action_space=A, debug_nonlinear='leaky_relu' if elu else 'relu')
    if app_dim:
        cfg.update(debug_core_appearance=True, debug_appearance_dim=app_dim)
    return cfg


def fill_factor(regime):
    """(base fill, k) of a regime: a committed fill by name, or ('scaled', k) -- 'init' with the reward head's weights times k"""
    return ('init', float(regime[1])) if isinstance(regime, tuple) else (regime, 1.0)


def case_regime(case, regime):
    """'spread' resolved for an expansion case"""
    return ('scaled', SPREAD_K[case.name]) if regime == 'spread' else regime


def scaled_value(name, shape, base, k, fan_in):
    """the float64 value of a parameter under (base, k)"""
    v = analytic_tensor(name, shape, torch.float64, base, fan_in)
    return v * k if (k != 1.0 and name in [n + '.weight' for n in RH_LAYERS]) else v


@functools.lru_cache(maxsize=None)
def _structs():
    return O.build_structs(O.default_config())


@functools.lru_cache(maxsize=None)
def plan_oracle(N, A, app_dim, elu, regime, dtype=torch.float64):
    """(config, the 'dyn.' parameters without autograd) of the oracle; shared, read-only"""
    c = O.default_config(**plan_cfg(N, A, app_dim, elu))
    shapes = {k: v for k, v in O.param_shapes(c, _structs()).items() if k.startswith('dyn.')}
    fi = fan_ins({k: tuple(v) for k, v in shapes.items()})
    base, k = fill_factor(regime)
    return c, {n: scaled_value(n, s, base, k, fi.get(n)).to(dtype) for n, s in shapes.items()}


def fill_module(module, prefix, regime):
    """the module's parameters under `regime`: the values of plan_oracle rounded to the parameters' dtype"""
    base, k = fill_factor(regime)
    with torch.no_grad():
        named = {prefix + n: p for n, p in module.named_parameters()}
        fi = fan_ins({n: tuple(p.shape) for n, p in named.items()})
        for n, p in named.items():
            p.copy_(scaled_value(n, p.shape, base, k, fi.get(n)).to(p.dtype))
    return module


def rh_packed(params):
    """the kernels' parameter block: the ten tensors one after the other, flat"""
    return torch.cat([params[n].reshape(-1) for n in RH_PACKED])


def rh_unpack(flat):
    """a block in the kernels' layout -> {name: tensor}"""
    shapes = {'0.0': (32, 32), '0.2': (32, 32), '1.0': (16, 32), '1.2': (8, 16), '1.4': (1, 8)}
    out, pos = {}, 0
    for n in RH_LAYERS:
        w = shapes[n[-3:]]
        for name, shp in ((n + '.weight', w), (n + '.bias', w[:1])):
            size = int(np.prod(shp))
            out[name] = flat[pos:pos + size].reshape(shp)
            pos += size
    assert pos == flat.numel()
    return out


# ------------------------------------------------------------------------------------------------ the reward head
def rh_preacts(params, pred):
    """the three ReLU layers' pre-activations: (B,N,32), (B,16), (B,8)"""
    p0 = O._lin(params, 'dyn.reward_head0.0', pred)
    q = O._lin(params, 'dyn.reward_head0.2', torch.relu(p0)).sum(1)
    p1 = O._lin(params, 'dyn.reward_head1.0', q)
    p2 = O._lin(params, 'dyn.reward_head1.2', torch.relu(p1))
    return p0, p1, p2


def relu_margins(pre, scales=None):
    """per item, the smallest |pre-activation| / its layer's largest over the three layers; scales: the largest per layer (default:
    of `pre` itself) -> (margin (B,), scales)"""
    flat = [p.abs().flatten(1) for p in pre]
    if scales is None:
        scales = [float(f.max()) for f in flat]
    return torch.stack([f.min(1).values / s for f, s in zip(flat, scales)]).min(0).values, scales


def relu_unit_use(pre):
    """per layer, the fraction of units that are active on some item and inactive on some item"""
    out = []
    for p in pre:
        on = (p > 0).reshape(-1, p.shape[-1])
        out.append(float((on.any(0) & (~on).any(0)).double().mean()))
    return out


def spread_conditions(rewards, pre):
    """the three conditions of the 'spread' fill on a case's float64 rewards and pre-activations -> (all hold, the figures)"""
    r = rewards.detach().flatten().numpy()
    q10, q90 = np.quantile(r, [0.1, 0.9])
    use = relu_unit_use(pre)
    fig = {'q10': float(q10), 'q90': float(q90), 'min': float(r.min()), 'max': float(r.max()), 'use': use}
    return bool(q90 - q10 >= 0.1 and r.min() > 0.02 and r.max() < 0.98 and min(use) >= 0.25), fig


def rh_reference(params, pred, d_reward, dtype=torch.float64):
    """O.reward_head forward and backward in `dtype`: dict(reward (items,), H0, Q, A1, A2, d_pred, grads {name: gradient})"""
    params = {k: v.detach().to(dtype).clone().requires_grad_() for k, v in params.items() if 'reward_head' in k}
    x = pred.detach().to(dtype).clone().requires_grad_()
    reward, h0, q, a1, a2 = O.reward_head(params, x, saved=True)
    (reward[:, 0] * d_reward.to(dtype)).sum().backward()
    return {'reward': reward.detach()[:, 0], 'H0': h0.detach(), 'Q': q.detach(), 'A1': a1.detach(), 'A2': a2.detach(), 'd_pred': x.grad,
            'grads': {k: p.grad for k, p in params.items()}}


RH_ITEMS_N3 = (1, 3, 4, 5, 1023, 1024, 1025, 2049)
RH_SHAPES = [(items, 3) for items in RH_ITEMS_N3] + [(items, n) for n in (1, 2, 4, 5, 6, 7, 8) for items in (5, 1025)]
RH_FILLS = ('init', 'spread', 'saturated')
RH_GRADS = ('drawn', 'third_zero', 'zero')
RH_PLANTS = (30.0, -30.0)


def rh_fills(items):
    """the fills a shape runs under: the saturated one where the draw is large enough to hold unsaturated items for certain -- its
    gradients are relative to THEIR scale, and the only item of a one-item case can be a saturated one"""
    return RH_FILLS if items >= 1000 else RH_FILLS[:2]


def rh_regime(fill, N):
    return {'saturated': ('scaled', RH_SATURATED_K), 'spread': ('scaled', RH_SPREAD_K[N])}.get(fill, fill)


@functools.lru_cache(maxsize=None)
def rh_params(N, fill, dtype=torch.float64):
    """the reward head under a fill (it does not depend on A or app_dim; N enters 'spread' through its factor)"""
    _, params = plan_oracle(N, 9, 3, False, rh_regime(fill, N), dtype)
    return {k: v for k, v in params.items() if 'reward_head' in k}


@functools.lru_cache(maxsize=None)
def rh_inputs(items, N):
    """pred (items,N,32), float32 values in float64: normal draws of the scale the dynamics core produces (0.5), +-30 planted in a few
    items; every item keeps RELU_MARGIN (twice that, against the scale of a first draw) under all of RH_FILLS -- items that do not
    are passed over, in the order drawn.  d_reward (items,) standard normal.  -> (pred, d_reward, items passed over)"""
    g = torch.Generator().manual_seed(31000 + 10 * items + N)
    fills = [rh_params(N, f) for f in RH_FILLS]

    stride = 1 if items < 8 else 8                       # every item of the shapes below eight items holds plants, every eighth above

    def draw(m):
        x = 0.5 * torch.randn(m, N, 32, generator=g, dtype=torch.float64)
        for i in range(0, m, stride):
            where = torch.randperm(N * 32, generator=g)[:2]
            x[i].view(-1)[where] = torch.tensor(RH_PLANTS, dtype=torch.float64)
        return x.float().double()
    scales = [relu_margins(rh_preacts(p, draw(512)))[1] for p in fills]
    keep, passed = [], 0
    while len(keep) < items:
        x = draw(items - len(keep) + 8)
        ok = torch.stack([relu_margins(rh_preacts(p, x), s)[0] > 2 * RELU_MARGIN for p, s in zip(fills, scales)]).all(0)
        for i in range(x.shape[0]):
            if len(keep) == items:
                break
            if ok[i]:
                keep.append(x[i])
            else:
                passed += 1
    d_reward = torch.randn(items, generator=g, dtype=torch.float64).float().double()
    return torch.stack(keep), d_reward, passed


def rh_spread_conditions(N, items=1025):
    """spread_conditions of the reward-head cases at N objects: on the `items`-item case (the smaller ones share its weights and cannot
    show a quantile or a unit in both states), over the items without a planted entry (a +-30 input saturates its item by design)"""
    pred = rh_inputs(items, N)[0]
    plain = (pred.abs() < min(abs(v) for v in RH_PLANTS)).flatten(1).all(1)
    params = rh_params(N, 'spread')
    return spread_conditions(O.reward_head(params, pred[plain]), rh_preacts(params, pred[plain]))


@functools.lru_cache(maxsize=None)
def rh_case_reference(items, N, fill, variant, dtype=torch.float64):
    """rh_reference of a reward-head case; computed once, shared, read-only"""
    return rh_reference(rh_params(N, fill, dtype), rh_inputs(items, N)[0], rh_d_reward(items, N, variant), dtype)


def rh_d_reward(items, N, variant):
    d = rh_inputs(items, N)[1].clone()
    if variant == 'third_zero':
        d[::3] = 0.0
    elif variant == 'zero':
        d.zero_()
    return d


# ------------------------------------------------------------------------------------------------ the expansion
STATE_SPAN = 0.9          # leaf states are drawn in [-span, span]
Case = collections.namedtuple('Case', 'name N A app M L D len_s elu cap leaf child span')


def _slots(M, A, cap, tight):
    """leaf and child slots per tree.  tight: the last legal ones -- leaf = cap - 1 / child = cap - A, alone and (every third tree)
    both at once, where child A - 1 lands on the leaf's own slot; else three placements inside a pool of 2 A + 3 slots"""
    pats = [(cap - 1, 0), (0, cap - A), (cap - 1, cap - A)] if tight else [(0, 1), (cap - 1, cap - 1 - A), (A + 2, 2)]
    return tuple(pats[m % 3][0] for m in range(M)), tuple(pats[m % 3][1] for m in range(M))


def _case(name, N, A, app, M, L, D, len_s=None, elu=False, cap=None, tight=False, span=None):
    cap = 2 * A + 3 if cap is None else cap
    len_s = tuple(1 + m % D for m in range(M)) if len_s is None else tuple(len_s)
    leaf, child = _slots(M, A, cap, tight)
    return Case('%s-N%d-A%d-app%d-M%d-L%d-%s' % (name, N, A, app, M, L, 'elu' if elu else 'lrelu'), N, A, app, M, L, D, len_s, elu, cap, leaf,
                child, STATE_SPAN if span is None else span)


def expansion_cases():
    out = [_case('counts', n, 9, 3, 3, 5, 3, elu=n in (1, 3, 5), tight=n in (1, 8)) for n in range(1, 9)]
    # (under the ELU core at six objects the rewards of 27 rows spread by a tenth only from leaf states drawn wider)
    out.append(_case('counts', 6, 9, 3, 3, 5, 3, elu=True, span=1.5))
    out += [_case('few', n, a, 3, 3, 5, 3, elu=(n, a) in ((2, 1), (5, 2)), cap=1 + a, tight=True) for n in (2, 5) for a in (1, 2)]
    out += [_case('limit', n, 64, 3, 17, 2, 3) for n in (2, 5)]                       # 1 088 rows; A L = 128
    out.append(_case('limit', 4, 64, 12, 2, 5, 3, elu=True))                          # A L = 320
    out.append(_case('rows', 3, 9, 3, 114, 2, 3))                                     # the workload's action count, 1 026 rows
    out += [_case('noapp', n, 9, 0, 3, 5, 3, elu=n != 4) for n in (1, 4, 7)]
    out += [_case('wide', n, 9, 12, 3, 5, 3, elu=True) for n in (3, 8)]
    out.append(_case('onestep', 3, 9, 3, 3, 1, 1))
    out.append(_case('long', 2, 2, 0, 2, 70, 40, len_s=(1, 25)))
    return out


def case_id(case):
    return case.name


def geometry(case):
    """the trip counts of csrc/plan.hip and csrc/capi.hip at a case, as read from the code"""
    rows = case.M * case.A
    blocks = min(max((rows + 3) // 4, 1), 256)                       # reward_head_blocks, kRhWaves = 4
    return {'rows': rows, 'zrow': case.N * 18, 'scatter_trips': -(-case.N * 18 // 64), 'AL': case.A * case.L,
            'index_trips': -(-case.A * case.L // 256), 'embed_trips': case.A, 'blocks': blocks, 'row_trips': -(-rows // (blocks * 4)),
            'nan_fill_trips': -(-case.L // 64), 'sin_dim': 20 + case.app, 'gnn_small': 2 <= case.N <= 6}


def one_hot_actions(acts, A, trees):
    """(trees A, 1 + L, A): action a of the row first, then its random actions"""
    first = torch.arange(A).repeat(trees)[:, None]
    return torch.nn.functional.one_hot(torch.cat([first, acts.long()], 1), A)


def oracle_rollout(c, params, z, app, acts, A):
    """O.rollout of every (tree, action) row: z (trees,N,18), app (trees,N,app_dim) or None, acts (trees A, L) -> zs (rows, 1 + L, N,
    18), rewards (rows, 1 + L), in the parameters' dtype"""
    dtype = next(iter(params.values())).dtype
    with torch.no_grad():
        zs, rew = O.rollout(c, params, z.repeat_interleave(A, 0).to(dtype), 1 + acts.shape[1], one_hot_actions(acts, A, z.shape[0]).to(dtype),
                            app.repeat_interleave(A, 0).to(dtype) if app is not None else None)
    return zs, rew[..., 0]


def rollout_preds(c, params, z, actions, app):
    """O.rollout's loop with the dynamics core's `pred` kept: z (B,N,18), actions (B,T,A) one-hot, app (B,N,app_dim) or None ->
    zs (B,T,N,18), rewards (B,T), preds (B,T,N,32)"""
    cl = c.cl
    zs, rews, preds, cur = [], [], [], z
    with torch.no_grad():
        for t in range(actions.shape[1]):
            out, rew, pred = O.dynamics_forward(c, params, cur[..., 2:], actions[:, t], app, with_pred=True)
            m, _ = O.constrain_z_dyn(c, out[..., :cl // 2], out[..., cl // 2:])
            cur = torch.cat([z[..., :2], cur[..., 2:4] + m[..., :2], m[..., 2:]], -1)
            zs.append(cur)
            rews.append(rew[:, 0])
            preds.append(pred)
    return torch.stack(zs, 1), torch.stack(rews, 1), torch.stack(preds, 1)


def value(rew, len_s, D, dtype, M, A, gamma=GAMMA):
    """the reference's backpropagate value, written out per row in `dtype`: rew (M A, 1 + L) -> (M, A)"""
    rew = rew.numpy().astype(dtype)
    L = rew.shape[1] - 1
    q = np.zeros((M, A), dtype=dtype)
    g = dtype(gamma)
    for m in range(M):
        n = min(2 * D - len_s[m] + 1, L)
        s2 = dtype(0)
        for j in range(len_s[m], D):
            s2 += g ** dtype(j)
        for a in range(A):
            r = rew[m * A + a]
            s1 = dtype(0)
            for k in range(n):
                s1 += r[1 + k] - dtype(1)
            q[m, a] = (r[0] - dtype(1)) * g ** dtype(len_s[m]) + s1 * s2
    return q


def draw_states(g, trees, N, app_dim, span=None):
    """leaf states (trees,N,18) -- scales in [0.1, 0.3], the rest in [-span, span] -- and appearances (trees,N,app_dim) in [0, 1] or
    None, float32 values in float64 (the draws of tests/test_gpu_plan.py, which have span 0.6: the wider one moves more of the reward
    head's units across zero)"""
    span = STATE_SPAN if span is None else span
    z = torch.cat([torch.rand(trees, N, 2, generator=g) * 0.2 + 0.1, (torch.rand(trees, N, 16, generator=g) * 2 - 1) * span], -1).double()
    app = torch.rand(trees, N, app_dim, generator=g).double() if app_dim else None
    return z, app


# seeds of make_inputs per (case name, regime); every smaller seed was passed over: on its draws the three conditions of the 'spread'
# fill held at no k of tools/make_plan_inputs.py's grid (seed 0 where a case is not listed)
INPUT_SEEDS = {
    ('counts-N3-A9-app3-M3-L5-elu', 'spread'): 3,
    ('counts-N5-A9-app3-M3-L5-elu', 'spread'): 4,
    ('counts-N6-A9-app3-M3-L5-elu', 'spread'): 4,
    ('counts-N7-A9-app3-M3-L5-lrelu', 'spread'): 8,
    ('counts-N8-A9-app3-M3-L5-lrelu', 'spread'): 14,
    ('limit-N4-A64-app12-M2-L5-elu', 'spread'): 3,
    ('noapp-N7-A9-app0-M3-L5-elu', 'spread'): 2,
    ('onestep-N3-A9-app3-M3-L1-lrelu', 'spread'): 1,
    ('wide-N8-A9-app12-M3-L5-elu', 'spread'): 2,
}


def _case_seed(case, regime):
    names = [c.name for c in expansion_cases()]
    return 52000 + 1000 * INPUT_SEEDS.get((case.name, regime), 0) + 10 * names.index(case.name) + REGIMES.index(regime)


def _margins_of(params, preds, scales):
    """preds (B,T,N,32) -> (B,T) margins"""
    B, T = preds.shape[:2]
    return relu_margins(rh_preacts(params, preds.flatten(0, 1)), scales)[0].view(B, T)


PILOT_STEPS = 6           # random actions of make_inputs' pilot draw (seven steps with the first)
LONG_HEADROOM = 1.5       # make_inputs_long: a row's largest pre-activation may be this many times the pilot rows' median


def make_inputs_long(case, regime, reject=True, pilot=256, batch=1024):
    """make_inputs for a rollout longer than its pilot.  Positions add up over the steps, so the late steps of a long rollout set the
    layers' largest (ten times the first steps' at L = 70): a margin against the first steps' scale says little, and a tree accepted
    on it leaves its rows no clear actions.  Here the scale per layer is LONG_HEADROOM times the median, over the rows of a
    full-length pilot, of the row's largest; a row counts as clear if it stays below that scale and keeps RELU_MARGIN of it away from
    zero over all its steps, so the case drawn has no larger scale.  A tree is drawn with `batch` rows of random actions at once and
    taken if every first action has a clear row (the first one is kept); else the tree is passed over with all its rows.
    -> (z, app, acts, (trees redrawn, rows redrawn))"""
    c, params = plan_oracle(case.N, case.A, case.app, case.elu, case_regime(case, regime))
    N, A, M, L = case.N, case.A, case.M, case.L
    g = torch.Generator().manual_seed(_case_seed(case, regime))

    def rows_of(z, app, trees, acts):
        """-> per layer the rows' largest |pre-activation| (rows,), and the pre-activations (rows, 1 + L, ...)"""
        _, _, p = rollout_preds(c, params, z.repeat_interleave(acts.shape[0] // trees, 0), one_hot_actions(acts, A, acts.shape[0] // A).double(),
                                app.repeat_interleave(acts.shape[0] // trees, 0) if app is not None else None)
        pre = [x.reshape(acts.shape[0], 1 + L, -1) for x in rh_preacts(params, p.flatten(0, 1))]
        return [x.abs().flatten(1).max(1).values for x in pre], pre
    z0, app0 = draw_states(g, pilot, N, case.app, case.span)
    largest, _ = rows_of(z0, app0, pilot, torch.randint(0, A, (pilot * A, L), generator=g))
    bound = [LONG_HEADROOM * float(x.median()) for x in largest]
    per = max(1, batch // A)                                     # rows per first action
    zs, apps, acts, trees_redrawn, rows_redrawn = [], [], [], 0, 0
    while len(zs) < M:
        z, app = draw_states(g, 1, N, case.app, case.span)
        cand = torch.randint(0, A, (per * A, L), generator=g)   # row i: first action i % A
        largest, pre = rows_of(z, app, 1, cand)
        ok = torch.stack([x <= b for x, b in zip(largest, bound)]).all(0)
        ok &= relu_margins([x.flatten(1) for x in pre], bound)[0] > RELU_MARGIN
        ok = (ok | (not reject)).view(per, A)
        if bool(ok.any(0).all()):
            pick = ok.double().argmax(0)                         # the first clear row of each first action
            zs.append(z[0])
            apps.append(app[0] if app is not None else None)
            acts.append(cand.view(per, A, L)[pick, torch.arange(A)])
            rows_redrawn += int(pick.sum())
        else:
            trees_redrawn += 1
            rows_redrawn += per * A
            assert trees_redrawn < 2000, 'no tree with clear rows: ' + case.name
    return torch.stack(zs), torch.stack(apps) if case.app else None, torch.cat(acts), (trees_redrawn, rows_redrawn)


def make_inputs(case, regime, chunk=4096, reject=True):
    """Draw the inputs of a case: z (M,N,18), app (M,N,app) or None, acts (M A, L), every ReLU pre-activation of the reward head clear
    of zero by 2 RELU_MARGIN of its layer's largest in a first plain draw of up to seven steps (the CPU test asserts RELU_MARGIN against the largest of
    the case itself).  -> (z, app, acts, (trees redrawn, rows redrawn))"""
    if case.L > PILOT_STEPS:          # the pilot below does not see the whole rollout
        return make_inputs_long(case, regime, reject)
    c, params = plan_oracle(case.N, case.A, case.app, case.elu, case_regime(case, regime))
    N, A, M, L = case.N, case.A, case.M, case.L
    g = torch.Generator().manual_seed(_case_seed(case, regime))
    margin = 2 * RELU_MARGIN          # against the layers' largest over the first seven steps of a plain draw
    z0, app0 = draw_states(g, 8, N, case.app, case.span)
    a0 = torch.randint(0, A, (8 * A, min(L, PILOT_STEPS)), generator=g)
    _, _, p = rollout_preds(c, params, z0.repeat_interleave(A, 0), one_hot_actions(a0, A, 8).double(),
                            app0.repeat_interleave(A, 0) if app0 is not None else None)
    scales = relu_margins(rh_preacts(params, p.flatten(0, 1)))[1]
    first = torch.nn.functional.one_hot(torch.arange(A), A).double()[:, None]              # (A, 1, A)
    if A == 1:                                            # one action: the rows have no random actions to redraw, the tree is the row
        first = first.expand(1, 1 + L, 1)
    zs, apps, trees_redrawn = [], [], 0
    K = max(1, chunk // A)
    while len(zs) < M:                                    # trees whose A first steps (A = 1: all steps) are clear
        z, app = draw_states(g, K, N, case.app, case.span)
        _, _, p = rollout_preds(c, params, z.repeat_interleave(A, 0), first.repeat(K, 1, 1),
                                app.repeat_interleave(A, 0) if app is not None else None)
        ok = (_margins_of(params, p, scales).view(K, -1) > margin).all(1) | (not reject)
        for k in range(K):
            if len(zs) == M:
                break
            if ok[k]:
                zs.append(z[k])
                apps.append(app[k] if app is not None else None)
            else:
                trees_redrawn += 1
    z = torch.stack(zs)
    app = torch.stack(apps) if case.app else None
    rows = M * A
    acts = torch.zeros(rows, L, dtype=torch.long)
    todo, rows_redrawn = torch.arange(rows), 0
    zr, appr = z.repeat_interleave(A, 0), app.repeat_interleave(A, 0) if app is not None else None
    row_first = torch.nn.functional.one_hot(torch.arange(A).repeat(M), A)[:, None]       # (rows, 1, A)
    for tries in range(12000):
        if not len(todo):
            break
        if tries and tries % 3000 == 0:       # rows that stay stuck (a long rollout settles wherever its tree sends it): another tree
            for m in sorted(set((todo // A).tolist())):
                while True:
                    zc, appc = draw_states(g, 1, N, case.app, case.span)
                    _, _, p = rollout_preds(c, params, zc.repeat_interleave(A, 0), first, appc.repeat_interleave(A, 0) if appc is not None else None)
                    trees_redrawn += 1
                    if bool((_margins_of(params, p, scales) > margin).all()):
                        break
                z[m] = zc[0]
                if app is not None:
                    app[m] = appc[0]
                todo = torch.unique(torch.cat([todo, torch.arange(m * A, (m + 1) * A)]))
            zr, appr = z.repeat_interleave(A, 0), app.repeat_interleave(A, 0) if app is not None else None
        cand = torch.randint(0, A, (len(todo), L), generator=g)
        ok = torch.zeros(len(todo), dtype=torch.bool)
        for s in range(0, len(todo), chunk):
            i = todo[s:s + chunk]
            oh = torch.cat([row_first[i], torch.nn.functional.one_hot(cand[s:s + chunk], A)], 1).double()
            _, _, p = rollout_preds(c, params, zr[i], oh, appr[i] if appr is not None else None)
            ok[s:s + chunk] = (_margins_of(params, p, scales) > margin).all(1) | (not reject)
        acts[todo[ok]] = cand[ok]
        rows_redrawn += int((~ok).sum())
        todo = todo[~ok]
    assert not len(todo), 'rows without clear random actions: ' + case.name
    return z, app, acts, (trees_redrawn, rows_redrawn)


_FIXTURE = None


def load_inputs(case, regime):
    """the committed inputs of a case -> (z (M,N,18), app (M,N,app) or None, acts (M A, L) int64), float32 values in float64"""
    global _FIXTURE
    if _FIXTURE is None:
        _FIXTURE = dict(np.load(FIXTURE))
    key = case.name + '/' + regime
    z = torch.from_numpy(_FIXTURE[key + '/z']).double()
    app = torch.from_numpy(_FIXTURE[key + '/app']).double() if case.app else None
    return z, app, torch.from_numpy(_FIXTURE[key + '/acts']).long()


@functools.lru_cache(maxsize=None)
def expansion_reference(case, regime, dtype=torch.float64):
    """O.rollout on the case's inputs and the value formula, in `dtype`: dict(z (rows,N,18) the child states, r (rows, 1 + L),
    q (M,A) numpy); computed once, shared, read-only"""
    c, params = plan_oracle(case.N, case.A, case.app, case.elu, case_regime(case, regime), dtype)
    z, app, acts = load_inputs(case, regime)
    zs, rew = oracle_rollout(c, params, z, app, acts, case.A)
    return {'z': zs[:, 0], 'r': rew, 'q': value(rew, case.len_s, case.D, np.float64 if dtype == torch.float64 else np.float32, case.M, case.A)}


@functools.lru_cache(maxsize=None)
def expansion_preacts(case, regime):
    """-> rewards (rows, 1 + L) and the reward head's float64 pre-activations over all rows and steps of a case"""
    return preacts_of(case, case_regime(case, regime), *load_inputs(case, regime))


def preacts_of(case, regime, z, app, acts):
    c, params = plan_oracle(case.N, case.A, case.app, case.elu, regime)
    _, rew, preds = rollout_preds(c, params, z.repeat_interleave(case.A, 0), one_hot_actions(acts, case.A, case.M).double(),
                                  app.repeat_interleave(case.A, 0) if app is not None else None)
    return rew, rh_preacts(params, preds.flatten(0, 1))


# ------------------------------------------------------------------------------------------------ the search
SearchCase = collections.namedtuple('SearchCase', 'N A M D R app seed')
# seeds chosen on the float64 oracle (search_on_oracle): the smallest decision gap over all trees and iterations is >= 1e-4;
# SEARCH_SEEDS_PASSED lists the seeds tried before, whose smallest gap was below that
SEARCH_CASES = [SearchCase(1, 1, 2, 2, 6, 3, 3), SearchCase(2, 64, 3, 2, 8, 3, 0), SearchCase(6, 2, 70, 4, 16, 3, 0), SearchCase(8, 9, 3, 5, 12, 3, 0)]
SEARCH_SEEDS_PASSED = {'N1-A1-M2-D2-R6': [0, 1, 2]}          # (the 'spread' conditions held at no k on the roots of these seeds)
SEARCH_GAP = 1e-4


def search_id(s):
    return 'N%d-A%d-M%d-D%d-R%d' % s[:5]


def search_inputs(s):
    """roots z (M,N,18), app (M,N,app) and every iteration's random-rollout actions (R, M A, 2 D) of a search case"""
    g = torch.Generator().manual_seed(77000 + 7919 * s.seed + 100 * s.N + s.A)
    z, app = draw_states(g, s.M, s.N, s.app)
    acts = torch.randint(0, s.A, (s.R, s.M * s.A, 2 * s.D), generator=g)
    return z, app, acts.numpy()


def search_root_expansion(s):
    """-> rewards and reward-head pre-activations of the first expansion of a search case (the 'spread' conditions are scored on it)"""
    z, app, acts = search_inputs(s)
    return preacts_of(_case('search', s.N, s.A, s.app, s.M, 2 * s.D, s.D), ('scaled', SEARCH_SPREAD_K[search_id(s)]), z, app,
                      torch.from_numpy(acts[0]))


def search_on_oracle(s, dtype=torch.float64):
    """The host Forest (stove_amd.mcts.mcts_stove) driven with the oracle's expansions on the CPU, `spread` weights: -> the forest
    after R iterations (forest.min_gap: the smallest decision gap) and the leaves selected (R, M)"""
    from stove_amd.mcts.mcts_stove import Forest, discounted_values
    c, params = plan_oracle(s.N, s.A, s.app, False, ('scaled', SEARCH_SPREAD_K[search_id(s)]), dtype)
    z, app, acts = search_inputs(s)
    f = Forest(s.M, s.A, s.D, cap=1 + s.A * s.R)
    pool = torch.zeros(s.M, f.cap, s.N, 18, dtype=dtype)
    pool[:, 0] = z.to(dtype)
    rows, leaves = np.arange(s.M), []
    for i in range(s.R):
        leaf = f.select()
        child = f.child_slots(leaf)
        len_s = f.depth[rows, leaf] + 1
        zs, rew = oracle_rollout(c, params, pool[rows, leaf], app, torch.from_numpy(acts[i]), s.A)
        for m in range(s.M):
            pool[m, child[m]:child[m] + s.A] = zs[m * s.A:(m + 1) * s.A, 0]
        r = rew.double().numpy().reshape(s.M, s.A, -1)
        f.backpropagate(leaf, child, discounted_values(r[..., 0], r[..., 1:], len_s, s.D, GAMMA))
        leaves.append(leaf.copy())
    return f, np.stack(leaves)


# ------------------------------------------------------------------------------------------------ bars
# the plain bars each quantity holds elsewhere (tests/test_gpu_plan.py: 3e-6; the element-wise and gradient bars of
# tests/test_gpu_encoder_counts.py), and the caps of the float32 gaps: twice the largest gap of the reference's own float32 run over
# the case list, measured on the CPU (tests/test_plan_cases_cpu.py asserts every gap below its cap)
BAR_PLAN = 3e-6
BAR_VALUE = 1e-6
BAR_GRAD = (1e-5, 3e-5, 1.2e-3)            # largest entry, l2, entry-wise (gpu_helpers.check_grad)
GAP_CAPS = {
    'expand.z': 6.62e-07,
    'expand.r_first': 2.54e-06,
    'expand.r_roll': 2.11e-06,
    'expand.q': 8.19e-07,
    'rh.reward': 2.69e-06,
    'rh.H0': 8.36e-07,
    'rh.Q': 5.44e-07,
    'rh.A1': 7.71e-07,
    'rh.A2': 5.55e-07,
    'rh.d_pred': 1.39e-04,
    'rh.grad': 5.14e-04,
    'rh.grad.l2': 5.14e-04,
    'rh.grad.small': 1.11e-02,
}


def write_fixture():
    out = {}
    for case in expansion_cases():
        for regime in REGIMES:
            z, app, acts, redrawn = make_inputs(case, regime)
            key = case.name + '/' + regime
            out[key + '/z'] = z.float().numpy()
            if app is not None:
                out[key + '/app'] = app.float().numpy()
            out[key + '/acts'] = acts.numpy().astype(np.int8)
            out[key + '/redrawn'] = np.asarray(redrawn, dtype=np.int32)
            print(key, 'trees / rows redrawn', redrawn, flush=True)
    np.savez_compressed(FIXTURE, **out)
