"""Shared helpers for the parity tests (oracle side)."""
import copy
import os

import numpy as np
import torch

import stove_oracle as O
from analytic_weights import analytic_tensor, fan_ins

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def load_golden(name):
    return dict(np.load(os.path.join(GOLDEN, name + '.npz')))


def oracle_setup(dtype=torch.float64, requires_grad=True, regime='analytic', **cfg):
    """config + SPN structures + analytic parameters (weight regime `regime`) keyed by reference state-dict names."""
    c = O.default_config(**cfg)
    structs = O.build_structs(c)
    shapes = O.param_shapes(c, structs)
    fi = fan_ins({k: tuple(v) for k, v in shapes.items()})
    params = {}
    for k, shp in shapes.items():
        t = analytic_tensor(k, shp, dtype, regime, fi.get(k))
        params[k] = t.requires_grad_() if requires_grad else t
    return c, structs, params


def t_(a, dtype=torch.float64):
    return torch.from_numpy(np.asarray(a)).to(dtype)


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def reference_at_codes(gold, regime, cfg, codes):
    """The float64 oracle (pinned to the reference on this very fixture, tests/test_oracle_goldens.py) evaluated AT the codes another
    implementation's recognition network produced: a dict with the golden fixture's keys (elbo, p_*, gn_*, g_*, roll_*), everything
    the oracle does not restate (bg / patch / overlap means) copied from `gold`.  For the 'stress' regime, whose six-step recursion and
    its gradients amplify a 1e-5 difference of the codes to 1e-4 in z and 1e-2 in the dynamics' gradients: the recognition network is
    held to the fixture's codes by its own test, everything behind it to the reference at the same codes."""
    dtype = torch.float64
    c, structs, params = oracle_setup(dtype, regime=regime, **cfg)
    x = t_(gold['x'], dtype)
    eps = {'latent': t_(gold['eps_lat'], dtype), 'std': t_(gold['eps_std'], dtype), 'steps': [t_(e, dtype) for e in gold['eps_steps']]}
    actions = t_(gold['actions'], dtype) if 'actions' in gold else None
    elbo, rewards, info = O.stove_forward(c, params, structs, x, eps, actions, detail=True, code_values=codes.detach().double().cpu())
    loss = -elbo
    if actions is not None:
        loss = loss + 3.0 * (rewards ** 2).sum()
    loss.backward()
    out = dict(gold)
    out['elbo'] = elbo.detach().numpy()
    for k in ('z', 'z_dyn', 'z_sup', 'z_std', 'z_sup_std', 'log_q', 'translik'):
        out['p_' + k] = info[k].detach().numpy()
    nan2 = np.full(2, np.nan)
    out['p_z_dyn_std'] = np.concatenate([nan2, info['z_dyn_std'].detach().numpy()])
    if actions is not None:
        out['rewards'] = rewards.detach().numpy()
        out['p_obj_appearances'] = info['obj_appearances'].detach().numpy()
    for k in list(gold):
        if k.startswith('gn_'):
            out[k] = params[k[3:]].grad.norm().numpy()
        elif k.startswith('g_'):
            out[k] = params[k[2:]].grad.numpy()
    with torch.no_grad():
        z_last = info['z'].detach()[:, -1]
        fut = actions[:, :5] if actions is not None else None
        app = info['obj_appearances'].detach()[:, -1] if actions is not None else None
        zp, rp = O.rollout(c, params, z_last, gold['roll_z'].shape[1], fut, app)
        out['roll_z'] = zp.numpy()
        if actions is not None:
            out['roll_rewards'] = rp.numpy()
        if 'eps_roll' in gold:
            zs, lq, _ = O.rollout(c, params, z_last, gold['roll_s_z'].shape[1], eps=[t_(e, dtype) for e in gold['eps_roll']])
            out['roll_s_z'], out['roll_s_logq'] = zs.numpy(), lq.numpy()
    return out


def source_index(z, zm, tol=1e-6):
    """idx[b, t, slot] = k with zm[b, t, slot] == z[b, t, k] (to `tol`): the permutation a matcher applied, recovered from its
    output; every matched row must be exactly one source row (rows of the test tracks differ in their first two columns)."""
    z, zm = torch.as_tensor(z).double().cpu(), torch.as_tensor(zm).double().cpu()
    eq = ((zm.unsqueeze(3) - z.unsqueeze(2)).abs() < tol).all(-1)
    assert bool((eq.sum(-1) == 1).all()), 'a matched row is not exactly one source row'
    return eq.long().argmax(-1)


def replica_index(n, K, seed=0):
    """src[row] = the distinct item (0 .. K-1) that row `row` of an n-row batch holds: item k on ceil / floor(n / K) rows (exactly
    R rows for n = K R), placed by a fixed random permutation.  The placement has no period and no block structure, so a kernel that
    reads row r +- s or row r mod m instead of row r reads another item on nearly every row (tests/test_batch_replication_cpu.py)."""
    g = np.random.default_rng(seed)
    return np.arange(n, dtype=np.int64)[g.permutation(n)] % K


def replica_counts(src, K):
    """how many rows hold each item: the factor of an item's share of a batch-summed gradient"""
    return np.bincount(np.asarray(src), minlength=K)


def oracle_stove(cfg, x, eps, actions=None, regime='analytic', dtype=torch.float64):
    """The float64 oracle's training step on one batch: loss = -ELBO (+ 3 mean(rewards^2) with actions, a batch mean like the ELBO,
    so that the loss of a replicated batch is the loss of its distinct sequences) -> dict(elbo, rewards, info, grads)."""
    c, structs, params = oracle_setup(dtype, regime=regime, **cfg)
    act = actions.to(dtype) if actions is not None else None
    eps = {'latent': eps['latent'].to(dtype), 'std': eps['std'].to(dtype), 'steps': [e.to(dtype) for e in eps['steps']]}
    elbo, rewards, info = O.stove_forward(c, params, structs, x.to(dtype), eps, act, detail=True)
    loss = -elbo
    if act is not None:
        loss = loss + 3.0 * (rewards ** 2).mean()
    loss.backward()
    return {'c': c, 'params': params, 'elbo': elbo.detach(), 'rewards': rewards.detach() if act is not None else None,
            'info': {k: (v.detach() if torch.is_tensor(v) else v) for k, v in info.items()},
            'grads': {k: p.grad for k, p in params.items() if p.grad is not None}}


def replicate_eps(eps, src):
    """the oracle's noise draws (O.draw_eps) of K sequences, row b of the result = row src[b]"""
    idx = torch.as_tensor(np.asarray(src))
    return {'latent': eps['latent'][idx], 'std': eps['std'][idx], 'steps': [e[idx] for e in eps['steps']]}


# ------------------------------------------------------------------------------------------------ dynamics at every object count
# Inputs of tests/test_oracle_counts_cpu.py and tests/test_gpu_dynamics_counts.py: drawn in float64 from a seeded CPU generator, nothing
# symmetric between the objects (every object its own position, scale and appearance row: a swapped or dropped edge changes the numbers).
DYN_VARIANTS = {
    'plain': {},                                                                            # cl/2 inputs per node
    'act': dict(action_conditioned=True, action_space=9),                                   # cl/2 + 4: actions without appearance
    'actapp': dict(action_conditioned=True, action_space=9, debug_core_appearance=True),    # cl/2 + 7
}


def dyn_width_cfg(cl):
    return {} if cl == 32 else dict(cl=cl, transition_lik_std=[0.01] * (cl // 2))


_DYN_ORACLES = {}


def dyn_oracle(cl, n_obj, variant, regime='analytic', dtype=torch.float64, nonlinear='relu'):
    """(config, the 'dyn.' parameters) of the oracle at one width / object count / input variant / weight regime: the parameters are
    built once and shared (they carry requires_grad; whoever differentiates clears their .grad first), the config is the caller's."""
    key = (cl, n_obj, variant, regime, dtype)
    if key not in _DYN_ORACLES:
        c, _, params = oracle_setup(dtype, regime=regime, num_obj=n_obj, **DYN_VARIANTS[variant], **dyn_width_cfg(cl))
        _DYN_ORACLES[key] = (c, {k: v for k, v in params.items() if k.startswith('dyn.')})
    c, params = _DYN_ORACLES[key]
    c = copy.copy(c)
    c.debug_nonlinear = nonlinear
    return c, params


def embed_actions(params, actions, n_obj):
    """one-hot actions (..., A) -> the action embedding's rows (..., n_obj, 4), as dynamics_forward appends them to the state"""
    return O._lin(params, 'dyn.action_embedding_layer', actions).view(*actions.shape[:-1], n_obj, 4)


def dyn_state(g, B, n_obj, cl, lo=-0.8, hi=0.8):
    """(B, N, cl/2) core inputs [x, y, vx, vy, latents] in [lo, hi]"""
    return torch.rand(B, n_obj, cl // 2, generator=g, dtype=torch.float64) * (hi - lo) + lo


def dyn_actions(g, variant, *lead):
    """one-hot actions (*lead, 9) in float64, or None for the plain variant"""
    if variant == 'plain':
        return None
    return torch.nn.functional.one_hot(torch.randint(0, 9, lead, generator=g), 9).double()


def dyn_appearance(g, variant, *lead):
    """appearance rows (*lead, 3) in [0, 1], or None"""
    return torch.rand(*lead, 3, generator=g, dtype=torch.float64) if variant == 'actapp' else None


def dyn_recursion_inputs(g, B, Ts, n_obj, cl):
    """-> z1 (B,N,cl/2+2), zsup, zsstd (B,Ts,N,6), eps (B,Ts,N,cl/2+2): scales in [0.15, 0.6], z1's positions in [-0.8, 0.8] (its
    velocities and latents in [-0.3, 0.3]), SuPAIR means in [-0.9, 0.9] with scales in [0.15, 0.6], stds in [0.02, 0.3]"""
    D = cl // 2
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)          # noqa: E731
    z1 = torch.cat([r(B, n_obj, 2) * 0.45 + 0.15, r(B, n_obj, 2) * 1.6 - 0.8, r(B, n_obj, D - 2) * 0.6 - 0.3], -1)
    zsup = torch.cat([r(B, Ts, n_obj, 2) * 0.45 + 0.15, r(B, Ts, n_obj, 4) * 1.8 - 0.9], -1)
    zsstd = r(B, Ts, n_obj, 6) * 0.28 + 0.02
    eps = torch.randn(B, Ts, n_obj, D + 2, generator=g, dtype=torch.float64)
    return z1, zsup, zsstd, eps


# ------------------------------------------------------------------------------------------------ state pipeline, z assembly, ELBO
# The float64 restatement of what csrc/state.hip computes, composed of the oracle's own functions, and the inputs of
# tests/test_state_chain_cpu.py and tests/test_gpu_state_counts.py.
STATE_SHAPES = [            # (n, T, skip): each hits one edge
    (1, 2, 1),              # no interior frame; skip = 1
    (1, 3, 2),              # one interior frame
    (3, 4, 3),              # T - skip = 1
    (6, 11, 2),             # the shape of test_state_pipeline_against_torch_chain: the anchor
    (5, 13, 5),             # several SuPAIR-scored frames
    (37, 9, 2),             # thread count no multiple of 256, several workgroups
    (2, 100, 2),            # (T - skip) o > 256 from o = 3 on: second trip of elbo_part_k's row loop; 99 likelihood entries per sequence
    (300, 3, 2),            # n > 256: second trip of elbo_final_k's loop
]
STATE_COUNTS = tuple(range(1, 9))          # 1 .. kMatchN, the limit stove_supair_state_fwd2 checks
STATE_MATCHERS = {'3_only': O.match_3only, 'greedy': O.match_greedy, 'volatile': O.match_volatile}
FIX_THRESHOLD, FIX_CLEARANCE, MATCH_MARGIN = 0.095, 1e-4, 1e-5


def state_cases():
    """(o, n, T, skip, mode, fix): every count x every shape x 'greedy' and 'volatile' ('3_only', too, at three objects); the
    smoothing stencil is off on a quarter of them, at every count, every shape and every mode"""
    out = []
    for o in STATE_COUNTS:
        for si, (n, T, skip) in enumerate(STATE_SHAPES):
            for mi, mode in enumerate(('greedy', 'volatile') + (('3_only',) if o == 3 else ())):
                out.append((o, n, T, skip, mode, (o + si + mi) % 4 != 0))
    return out


def state_case_id(case):
    return 'o%d-n%d-T%d-skip%d-%s-%s' % (case[:5] + ('fix' if case[5] else 'nofix',))


def state_config(o, skip=2, **kw):
    return O.default_config(num_obj=o, skip=skip, **kw)


def state_span_low(c):
    """the 8 spans and 8 lows of constrain_zp: the launch constants of the fused pipeline (Supair.zp_span_low)"""
    span = [c.max_obj_scale - c.min_obj_scale, c.max_y_scale - c.min_y_scale, 2 * c.obj_pos_bound, 2 * c.obj_pos_bound,
            c.scale_var, c.scale_var, c.pos_var, c.pos_var]
    return span + [c.min_obj_scale, c.min_y_scale, -c.obj_pos_bound, -c.obj_pos_bound, 0.0, 0.0, 0.0, 0.0]


def state_last_stage(zm, skip, fix, lat_noise=None):
    """matched states zm (n, T, o, 8) = [mean 4 | std 4] -> fix_supair, velocities, the recursion's inputs:
    zfix (n,T,o,8), hits (n,T,o) the two-bit mask of the dims whose jump to BOTH neighbours exceeds the threshold (0 with fix off),
    zl / sl (n,T-skip,o,6), init (n,o,6 [+ L]) = z_sup_full[:, skip-1] [| 0.01 lat_noise], jump (n,T-1,o,2) = |dz| of dims 0, 1"""
    z, s = zm[..., :4], zm[..., 4:]
    jump = (z[:, 1:, :, :2] - z[:, :-1, :, :2]).abs().detach()
    pad = torch.zeros_like(jump[:, :1])
    both = (torch.cat([pad, jump], 1) > FIX_THRESHOLD) & (torch.cat([jump, pad], 1) > FIX_THRESHOLD)
    hits = both[..., 0].long() + 2 * both[..., 1].long()
    if fix:
        z, s = O.fix_supair(z, s)
    else:
        hits = torch.zeros_like(hits)
    full, sfull = O.v_from_state(z), O.v_std_from_pos(s)
    init = full[:, skip - 1]
    if lat_noise is not None:
        init = torch.cat([init, 0.01 * lat_noise.to(init.dtype)], -1)
    return {'zfix': torch.cat([z, s], -1), 'hits': hits, 'zl': full[:, skip:], 'sl': sfull[:, skip:], 'init': init, 'jump': jump}


def state_chain(c, codes, n, T, o, skip, fix, mode, lat_noise=None):
    """constrain_zp -> matcher -> fix_supair -> v_from_state / v_std_from_pos in the dtype of `codes` (M, 8), differentiable:
    state_last_stage's dict plus zc (n,T,o,8), pos (n,T,o,2) and idx (n,T,o), the source object of every slot"""
    c = copy.copy(c)
    c.num_obj = o
    mean, std = O.constrain_zp(c, codes.reshape(-1, 8))
    zc = torch.cat([mean, std], -1).view(n, T, o, 8)
    zm, sm, _ = STATE_MATCHERS[mode](c, zc[..., :4], zc[..., 4:], None)
    zm = torch.cat([zm, sm], -1)
    out = state_last_stage(zm, skip, fix, lat_noise)
    out.update(zc=zc, pos=zc[..., 2:4], idx=source_index(zc.detach(), zm.detach(), 1e-9 if zc.dtype == torch.float64 else 1e-5))
    return out


def gather_slots(zc, idx):
    """zc (n,T,o,F), idx (n,T,o) -> out[b,t,k] = zc[b,t,idx[b,t,k]]"""
    return torch.gather(zc, 2, idx.unsqueeze(-1).expand(-1, -1, -1, zc.shape[-1]))


def match_walk(pos, mode):
    """The matchers' decisions on positions pos (n,T,o,2), frame by frame in pos.dtype, with what each decision won by:
    -> idx (n,T,o) (slot k of frame t holds object idx[b,t,k] of that frame), margin (n,) = the smallest cost margin of any decision
    of the sequence in the matchers' units (squared distance of (pos + 1) / 2); inf where nothing is decided.
    'greedy': smallest against second-smallest remaining entry, every round but the last (one entry left);
    'volatile': every slot's nearest current object against the runner-up;
    '3_only': the row minima, and in the repair path the pick of every row among the columns still free."""
    f = (pos + 1) / 2
    n, T, o, _ = f.shape
    rows, inf = torch.arange(n), float('inf')
    idx = [torch.arange(o).expand(n, o)]
    margin = torch.full((n,), inf, dtype=pos.dtype)

    def gap(e, seqs=None):                      # e (m, ..., candidates): the closest call among the leading dims, per sequence
        nonlocal margin
        if e.shape[-1] < 2:
            return
        two = e.topk(2, dim=-1, largest=False).values
        g = (two[..., 1] - two[..., 0]).reshape(e.shape[0], -1).min(1).values
        if seqs is None:
            margin = torch.minimum(margin, g)
        else:
            margin[seqs] = torch.minimum(margin[seqs], g)

    for t in range(1, T):
        prev, cur = torch.gather(f[:, t - 1], 1, idx[-1].unsqueeze(-1).expand(-1, -1, 2)), f[:, t]
        err = ((prev.unsqueeze(2) - cur.unsqueeze(1)) ** 2).sum(-1)             # [b, slot a, current object j]
        if mode == 'volatile':
            gap(err)
            pick = err.argmin(2)
        elif mode == 'greedy':
            e, pick = err.clone(), torch.zeros(n, o, dtype=torch.long)
            for r in range(o):
                flat = e.view(n, -1)
                if r < o - 1:
                    gap(flat)
                m = flat.argmin(1)
                a, j = m // o, m % o
                pick[rows, a] = j
                e[rows, a, :] = inf
                e[rows, :, j] = inf
        else:
            assert o == 3
            gap(err)
            pick = err.argmin(2).clone()
            bad = ~((pick[:, 0] != pick[:, 1]) & (pick[:, 1] != pick[:, 2]) & (pick[:, 0] != pick[:, 2]))
            if bad.any():
                fe, seqs = err[bad].clone(), bad.nonzero().flatten()
                for r in range(3):
                    gap(fe[:, r], seqs)
                    s = fe[:, r].argmin(-1)
                    pick[seqs, r] = s
                    fe[torch.arange(len(seqs)), :, s] = 1e12
        idx.append(pick)
    return torch.stack(idx, 1), margin


def state_conditions(zc, mode):
    """per sequence of constrained states zc (n,T,o,8): (idx, clearance (n,), margin (n,)) -- clearance = how far the nearest |jump|
    of the matched track's dims 0, 1 lies from the smoothing threshold, margin = match_walk's.  A sequence is usable by the float32
    kernels where clearance > FIX_CLEARANCE and margin > MATCH_MARGIN: both are discontinuities, and the device sees the float32 codes."""
    idx, margin = match_walk(zc[..., 2:4], mode)
    zm = gather_slots(zc[..., :2], idx)
    jump = (zm[:, 1:] - zm[:, :-1]).abs()
    return idx, (jump - FIX_THRESHOLD).abs().flatten(1).min(1).values, margin


def draw_codes(g, n, T, o):
    """recognition-network codes (n, T, o, 8), float32 values in float64: every track has a base code in [-6, 6] per dim (both tails
    of the sigmoid) that the frames jitter around; half the size codes (dims 0, 1) are redrawn per frame -- glitches for fix_supair,
    alone and in runs; the position codes walk at random around a base in [-3, 3], so that tracks cross; every frame lists its
    objects in an order of its own, which the matchers have to undo"""
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)          # noqa: E731
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)        # noqa: E731
    base = r(n, 1, o, 8) * 12 - 6
    codes = base + 0.05 * rn(n, T, o, 8)
    codes[..., :2] = torch.where(r(n, T, o, 2) < 0.5, r(n, T, o, 2) * 12 - 6, codes[..., :2])
    walk, steps = [rn(n, o, 2)], 0.6 * rn(n, T, o, 2)
    for t in range(1, T):
        walk.append(0.9 * walk[-1] + steps[:, t])               # (mean-reverting: a free walk of 100 frames ends in the sigmoid's tails,
    codes[..., 2:4] = 0.5 * base[..., 2:4] + torch.stack(walk, 1)      #  all objects in the corners of the frame)
    order = torch.argsort(r(n, T, o), -1)
    return gather_slots(codes, order).float().double()


def _accept(g, n, draw, usable, what):
    """The first n sequences of draw(g, m) -> tuple of (m, ...) tensors, in the order drawn, that usable(batch) -> bool (m,) accepts:
    the seeded choice of inputs that meet the stated conditions (never a skipped case) -> n tuples of per-sequence tensors"""
    keep = []
    for _ in range(400):
        cand = draw(g, 2 * (n - len(keep)) + 6)
        keep += [tuple(t[k] for t in cand) for k in usable(cand).nonzero().flatten().tolist()]
        if len(keep) >= n:
            return keep[:n]
    raise AssertionError('no inputs that meet the conditions: ' + what)


_STATE_INPUTS = {}


def state_inputs(case):
    """codes (n,T,o,8) of a case of state_cases(), float32 values in float64, every sequence of which meets state_conditions for the
    case's matcher (drawn once per case and shared)"""
    if case not in _STATE_INPUTS:
        o, n, T, skip, mode, fix = case
        c = state_config(o, skip)
        g = torch.Generator().manual_seed(700000 + 10000 * o + 100 * STATE_SHAPES.index((n, T, skip)) + list(STATE_MATCHERS).index(mode))

        def usable(cand):
            mean, std = O.constrain_zp(c, cand[0].reshape(-1, 8))
            _, clear, margin = state_conditions(torch.cat([mean, std], -1).view(-1, T, o, 8), mode)
            return (clear > FIX_CLEARANCE) & (margin > MATCH_MARGIN)
        seqs = _accept(g, n, lambda g_, m: (draw_codes(g_, m, T, o),), usable, state_case_id(case))
        _STATE_INPUTS[case] = torch.stack([s[0] for s in seqs])
    return _STATE_INPUTS[case]


def assert_state_conditions(ref, mode):
    """the stated input conditions on the reference side: ref = state_chain(...) in float64.  match_walk must have taken the oracle
    matcher's own decisions -- that is what makes its margins the margins of the reference."""
    idx, clear, margin = state_conditions(ref['zc'].detach(), mode)
    assert torch.equal(idx, ref['idx']), 'match_walk and the oracle matcher disagree'
    assert float((ref['jump'] - FIX_THRESHOLD).abs().min()) > FIX_CLEARANCE and float(clear.min()) > FIX_CLEARANCE
    assert float(margin.min()) > MATCH_MARGIN


STATE_IDX_FORMS = ('identity', 'permutation', 'volatile')


def given_idx_inputs(o, n, T, form, seed):
    """(zc (n,T,o,8), idx (n,T,o)) for the last stage alone: constrained states of draw_codes and a matching of the caller's --
    the identity, a random permutation per frame, or a non-permutation per frame (o >= 2: every frame names at least one object
    twice and leaves at least one out, what 'volatile' produces) -- whose gathered track keeps clear of the smoothing threshold"""
    assert form in STATE_IDX_FORMS and (form != 'volatile' or o >= 2)
    c = state_config(o)
    g = torch.Generator().manual_seed(seed)

    def draw(g_, m):
        mean, std = O.constrain_zp(c, draw_codes(g_, m, T, o).reshape(-1, 8))
        zc = torch.cat([mean, std], -1).view(m, T, o, 8).float().double()
        if form == 'identity':
            idx = torch.arange(o).expand(m, T, o).clone()
        elif form == 'permutation':
            idx = torch.argsort(torch.rand(m, T, o, generator=g_), -1)
        else:
            idx = torch.randint(0, o, (m, T, o), generator=g_)
            dup = torch.randint(0, o - 1, (m, T), generator=g_)
            idx.scatter_(2, (dup + 1).unsqueeze(-1), torch.gather(idx, 2, dup.unsqueeze(-1)))        # slot dup + 1 repeats slot dup
        return zc, idx

    def usable(cand):
        zm = gather_slots(cand[0][..., :2], cand[1])
        return ((zm[:, 1:] - zm[:, :-1]).abs() - FIX_THRESHOLD).abs().flatten(1).min(1).values > FIX_CLEARANCE
    pairs = _accept(g, n, draw, usable, 'given idx o%d n%d T%d %s' % (o, n, T, form))
    return torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])


def zall_chain(zfix, zs, skip):
    """z of the scene likelihood: the SuPAIR means of frames 1 .. skip-1, then the sampled states, [sx, sy/sx, x, y] -> [sx, sy, x, y]
    -> (n (T-1) o, 4)"""
    return O.sy_from_quotient(torch.cat([zfix[:, 1:skip, :, :4], zs[..., :4]], 1)).flatten(0, 2)


def elbo_chain(zs, mean, std, zdyn, lik, tstd, skip):
    """-> (ELBO, mean transition likelihood, mean log q) as Stove.forward assembles them; the mean over the SuPAIR-scored frames of an
    empty set (skip = 1) is taken as 0, as elbo_final_k states (torch.mean would give nan)"""
    logq = O.normal_log_prob(zs, mean, std).sum((-2, -1)).flatten()
    t = torch.as_tensor(tstd, dtype=zs.dtype).view(1, 1, 1, -1)
    trans = O.normal_log_prob(zs[..., 2:], zdyn, t).sum((-2, -1)).flatten()
    elbo = torch.mean(trans + lik[:, skip - 1:].reshape(-1) - logq)
    if skip > 1:
        elbo = elbo + torch.mean(lik[:, :skip - 1])
    return elbo, trans.mean(), logq.mean()


def elbo_inputs(g, n, T, o, skip, tstd, std_low=0.05):
    """float32 values in float64: q(z) means in [-1, 1], stds in [std_low, std_low + 0.5], z a draw from q, the dynamics' prediction
    within a few transition stds of z (so that no term of the ELBO drowns the others), likelihoods of +-200"""
    Ts = T - skip
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)          # noqa: E731
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)        # noqa: E731
    mean, std = r(n, Ts, o, 18) * 2 - 1, std_low + 0.5 * r(n, Ts, o, 18)
    std.view(-1)[0] = std_low
    zs = mean + std * rn(n, Ts, o, 18)
    zdyn = zs[..., 2:] + 1.5 * torch.as_tensor(tstd, dtype=torch.float64) * rn(n, Ts, o, 16)
    lik = 200.0 * rn(n, T - 1)
    return [t.float().double() for t in (zs, mean, std, zdyn, lik)]


_STATE_REFS = {}


def state_reference(case):
    """state_chain of a case on its state_inputs in float64, without autograd history; computed once and shared -- treat as read-only"""
    if case not in _STATE_REFS:
        o, n, T, skip, mode, fix = case
        with torch.no_grad():
            _STATE_REFS[case] = state_chain(state_config(o, skip), state_inputs(case).reshape(-1, 8), n, T, o, skip, fix, mode)
    return _STATE_REFS[case]


def state_coverage(cases):
    """what the references of `cases` show between them: the hit masks seen, whether two smoothed frames follow one another on a slot,
    whether a frame was smoothed at t = skip - 1 and at t = skip, and the counts at which 'volatile' gave a non-permutation"""
    cov = {'masks': set(), 'adjacent': False, 'at_skip_m1': False, 'at_skip': False, 'volatile_nonperm': set()}
    for case in cases:
        o, n, T, skip, mode, fix = case
        ref = state_reference(case)
        h = ref['hits']
        cov['masks'] |= set(h.unique().tolist())
        cov['adjacent'] |= bool(((h[:, 1:] > 0) & (h[:, :-1] > 0)).any())
        cov['at_skip_m1'] |= bool((h[:, skip - 1] > 0).any())
        cov['at_skip'] |= bool((h[:, skip] > 0).any())
        if mode == 'volatile' and bool((ref['idx'].sort(-1).values != torch.arange(o)).any()):
            cov['volatile_nonperm'].add(o)
    return cov


def assert_state_coverage(cov):
    assert cov['masks'] >= {0, 1, 2, 3}, cov['masks']
    assert cov['adjacent'] and cov['at_skip_m1'] and cov['at_skip'], cov
    assert cov['volatile_nonperm'] >= set(STATE_COUNTS[1:]), cov['volatile_nonperm']
