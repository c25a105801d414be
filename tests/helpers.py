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


# ------------------------------------------------------------------------------------------------ recognition network at every count
# The float64 restatement of what csrc/lstm.hip computes and the inputs / case lists of tests/test_encoder_counts_cpu.py and
# tests/test_gpu_encoder_counts.py.
def lstm_cell(pre, rec=None, c_prev=None):
    """One LSTM cell step in the dtype of `pre`, the lines of O.encoder_forward's loop: pre (n,4H) the pre-activation sum (gate order
    i, f, g, o), rec (n,4H) an optional recurrent term added to it, c_prev (n,H) the previous cell or None (zero) -> (c, h)"""
    gates = pre if rec is None else pre + rec
    i, f, g, o = gates.chunk(4, 1)
    cell = gates.new_zeros(i.shape) if c_prev is None else c_prev
    cell = torch.sigmoid(f) * cell + torch.sigmoid(i) * torch.tanh(g)
    return cell, torch.sigmoid(o) * torch.tanh(cell)


def lstm_cell_grads(pre, rec, c_prev, dh, dc_in=None):
    """lstm_cell and its backward through autograd, in the dtype of `pre`: dh (n,H) the gradient of h, dc_in (n,H) the gradient flowing
    into c from the next step or None -> dict(c, h, dg (n,4H) the gradient of the gate sum, dc_prev (n,H) the gradient of c_prev)"""
    gates = (pre if rec is None else pre + rec).detach().clone().requires_grad_()
    # no previous cell = a zero one: the same c and h, and its gradient dc sigmoid(f) exists either way (the kernel writes it either way)
    cp = (torch.zeros_like(dh) if c_prev is None else c_prev.detach().clone()).requires_grad_()
    c, h = lstm_cell(gates, None, cp)
    loss = (h * dh).sum()
    if dc_in is not None:
        loss = loss + (c * dc_in).sum()
    loss.backward()
    return {'c': c.detach(), 'h': h.detach(), 'dg': gates.grad, 'dc_prev': cp.grad}


def lstm_chain(x_proj, w_hh, steps):
    """`steps` cell steps on the same input projection x_proj (n,4H) = x W_ih^T + b: hs (n, steps, H).  Step 0 has neither a
    recurrent term nor a previous cell, as the kernels run it."""
    hs, h, c = [], None, None
    for _ in range(steps):
        c, h = lstm_cell(x_proj, None if h is None else h @ w_hh.t(), c)
        hs.append(h)
    return torch.stack(hs, 1)


CELL_SHAPES = [(1, 4), (3, 8), (37, 256), (257, 52), (2049, 256)]   # one thread / partial workgroup / ragged tails / H % 64 != 0
CELL_PLANTS = (30.0, -30.0, 100.0, -100.0, 1e-4, -1e-4)             # both tails of both activations, and small arguments
CELL_FAST = (0, 1)
CELL_MORE = 7                                                       # gate-gradient slabs of other steps: eight steps at most
CELL_FWD_FORMS = [(cp, gh) for cp in (False, True) for gh in (False, True)]                   # (c_prev given, gh given)
CELL_REF_FORMS = [(gh, cp, dc) for gh in (False, True) for cp in (False, True) for dc in (False, True)]
CELL_OUT_FORMS = [(True, None), (False, None), (True, 0), (False, 1), (True, 7)]            # (dg stored, dgx_sum: None or n_more)
CELL_BWD_FORMS = [r + o for r in CELL_REF_FORMS for o in CELL_OUT_FORMS]                      # (gh, c_prev, dc_in, dg, n_more)
_CELL_INPUTS, _CELL_REFS = {}, {}


def cell_inputs(n, H):
    """float32 values in float64, seeded per shape: gx, gh (n,4H) in [-3, 3] with CELL_PLANTS planted at drawn places of each, c_prev
    (n,H) in [-2, 2], dh, dc_in (n,H) and dg_more (CELL_MORE,n,4H) in [-1, 1] (drawn once per shape and shared: read-only)"""
    if (n, H) not in _CELL_INPUTS:
        g = torch.Generator().manual_seed(5000 + 97 * n + H)
        u = lambda lo, hi, *s: (torch.rand(*s, generator=g, dtype=torch.float64) * (hi - lo) + lo).float().double()      # noqa: E731
        x = {'gx': u(-3, 3, n, 4 * H), 'gh': u(-3, 3, n, 4 * H), 'c_prev': u(-2, 2, n, H), 'dh': u(-1, 1, n, H), 'dc_in': u(-1, 1, n, H),
             'dg_more': u(-1, 1, CELL_MORE, n, 4 * H)}
        copies = max(1, min(n * 4 * H // 64, 16))
        for k in ('gx', 'gh'):
            where = torch.randperm(n * 4 * H, generator=g)[:copies * len(CELL_PLANTS)]
            x[k].view(-1)[where] = torch.tensor(CELL_PLANTS, dtype=torch.float64).float().double().repeat(copies)
        _CELL_INPUTS[(n, H)] = x
    return _CELL_INPUTS[(n, H)]


def cell_reference(n, H, gh, cp, dc, dtype=torch.float64):
    """lstm_cell_grads on cell_inputs(n, H) with the recurrent term, the previous cell and the incoming cell gradient given or not
    (computed once per form and dtype, shared, read-only); dtype float32: the restatement's own float32 run, for the gap"""
    key = (n, H, gh, cp, dc, dtype)
    if key not in _CELL_REFS:
        x = {k: v.to(dtype) for k, v in cell_inputs(n, H).items()}
        _CELL_REFS[key] = lstm_cell_grads(x['gx'], x['gh'] if gh else None, x['c_prev'] if cp else None, x['dh'], x['dc_in'] if dc else None)
    return _CELL_REFS[key]


ENC_COUNTS = tuple(range(1, 9))
ENC_ROWS = (1, 37, 256, 300)          # below / on / above a 256-row tile; 1 and 37 are no multiple of 4 (weight gradients leave the MFMA kernel)
ENC_GEMMS = ('bf16x3', 'fp32')
ENC_REGIMES = ('analytic', 'init', 'stress')
ENC_D, ENC_H = 1024, 256


def encoder_cases():
    """(K, rows, regime, gemm, arena): the full cross"""
    return [(K, rows, regime, gemm, arena) for K in ENC_COUNTS for rows in ENC_ROWS for regime in ENC_REGIMES for gemm in ENC_GEMMS
            for arena in (True, False)]


def encoder_dx_cases():
    """(K, rows, regime, gemm): one case per K through ops.encoder_lstm with the gradient of the input asked for"""
    return [(K, 40, ENC_REGIMES[K % 3], 'bf16x3') for K in ENC_COUNTS]


def encoder_product_paths(rows, gemm, arena, needs_dx=False, gemm_ok=None):
    """Which kernels the products of _EncoderLstmFn take at a row count: 'mfma' (csrc/gemm_bf16.hip) or 'library'.
    forward (x W_ih^T, h W_hh^T) and dh (dg W_hh): the MFMA kernel unless gemm = 'fp32' -- their float4 sizes are 1024 and 256;
    wgrad (dW_ih, dW_hh): over `rows`, so the MFMA kernel only where rows % 4 == 0; direct: gradients added into the arena's views
    inside the kernels (needs the MFMA weight-gradient path and no gradient of the input)"""
    ok = gemm_ok if gemm_ok is not None else (lambda *d: all(int(v) % 4 == 0 and int(v) > 0 for v in d))
    mfma = gemm != 'fp32' and ok(ENC_D, ENC_H)
    wgrad = mfma and ok(rows)
    return {'forward': 'mfma' if mfma else 'library', 'dh': 'mfma' if mfma else 'library', 'wgrad': 'mfma' if wgrad else 'library',
            'direct': bool(arena and wgrad and not needs_dx)}


_ENC_INPUTS, _ENC_REFS = {}, {}


def encoder_inputs(K, rows):
    """frames (rows,1,32,32) in [0, 1] and an output weighting (rows,K,8) in [0, 1], float32 values in float64"""
    if (K, rows) not in _ENC_INPUTS:
        g = torch.Generator().manual_seed(9000 + 10 * rows + K)
        _ENC_INPUTS[(K, rows)] = (torch.rand(rows, 1, 32, 32, generator=g, dtype=torch.float64).float().double(),
                                  torch.rand(rows, K, 8, generator=g, dtype=torch.float64).float().double())
    return _ENC_INPUTS[(K, rows)]


def encoder_reference(K, rows, regime, dtype=torch.float64):
    """O.encoder_forward + backward under the output weighting: dict(codes, hs, grads {name without 'sup.encoder.': grad}); once per
    (K, rows, regime, dtype), shared, read-only.  float32: the oracle's own float32 run, for the gap."""
    key = (K, rows, regime, dtype)
    if key not in _ENC_REFS:
        c, _, params = oracle_setup(dtype, regime=regime, num_obj=K)
        params = {k: v for k, v in params.items() if k.startswith('sup.encoder.')}
        x, w = (t.to(dtype) for t in encoder_inputs(K, rows))
        codes, hs = O.encoder_forward(c, params, x, hidden=True)
        (codes * w).sum().backward()
        _ENC_REFS[key] = {'codes': codes.detach(), 'hs': hs.detach(), 'grads': {k[len('sup.encoder.'):]: p.grad for k, p in params.items()}}
    return _ENC_REFS[key]


COLSUM_ROWS = (0, 1, 15, 16, 17, 511, 512, 513, 8193)     # the level boundaries of colsum_level: <= 16 chunks, <= 512, a second level
COLSUM_COLS = (1, 3, 8, 50, 64, 68, 1024)                 # the narrow kernel (padded powers of two) and the float4 kernel
CHUNK_SIZES, CHUNK_COUNTS = (4, 1028), (1, 2, 16, 17)


def sum_inputs(seed, *shape):
    """float32 values in float64 in [-0.5, 1]: sums that grow with the row count, so the max norm has a scale"""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g, dtype=torch.float64) * 1.5 - 0.5).float().double()


# ------------------------------------------------------------------------------------------------ the assembled model at every count
MODEL_COUNTS = tuple(range(1, 9))
MODEL_SHAPES = ((3, 5), (1, 3))                  # (B, T); one sequence and a single recursion step in the second
MODEL_INIT_COUNTS = (1, 4, 8)


def model_cfg(N):
    """CASES['n6'] of tests/test_gpu_dynamics.py taken to every count: 'greedy' outside three objects, the six-object overlap weight
    and object scale above three"""
    cfg = dict(num_obj=N)
    if N != 3:
        cfg['debug_match_objects'] = 'greedy'
    if N > 3:
        cfg.update(overlap_beta=100.0, max_obj_scale=0.22)
    return cfg


def model_cases():
    """(N, B, T, regime, fused): every count x both shapes x the fused dynamics / state / ELBO switches on and off under the
    'analytic' weights, and the 'init' weights at 1, 4 and 8 objects (the flat parameter arena is on in all of them)"""
    return [(N, B, T, regime, fused) for N in MODEL_COUNTS for B, T in MODEL_SHAPES
            for regime in (('analytic', 'init') if N in MODEL_INIT_COUNTS else ('analytic',)) for fused in (True, False)]


def model_case_id(case):
    return 'N%d-B%dT%d-%s-%s' % (case[:4] + ('fused' if case[4] else 'opbyop',))


def paint_discs(centres, radii, res=32):
    """Frames of 1 .. 8 discs: centres (..., N, 2) = (x, y) in [-1, 1] frame coordinates, radii (N,) in pixels -> (..., 3, res, res)
    float32 values in float64, object k in colour channel k % 3, clipped to [0, 1].  A disc is 1 inside, 0 outside and falls
    linearly over the one pixel around its rim (so a sub-pixel move changes the frame)."""
    centres = np.asarray(centres, dtype=np.float64)
    N = centres.shape[-2]
    pix = np.arange(res, dtype=np.float64) + 0.5
    yy, xx = np.meshgrid(pix, pix, indexing='ij')
    out = np.zeros(centres.shape[:-2] + (3, res, res))
    for k in range(N):
        cx = (centres[..., k, 0] + 1) / 2 * res
        cy = (centres[..., k, 1] + 1) / 2 * res
        d = np.sqrt((xx - cx[..., None, None]) ** 2 + (yy - cy[..., None, None]) ** 2)
        out[..., k % 3, :, :] += np.clip(radii[k] + 0.5 - d, 0.0, 1.0)
    return torch.from_numpy(np.clip(out, 0.0, 1.0)).float().double()


def disc_radii(N):
    """every object its own radius (pixels): a swapped or dropped object changes the frame"""
    return (2.4 if N <= 3 else 1.6) + 0.3 * np.arange(N)


def draw_tracks(g, m, T, N):
    """m sequences of N disc centres over T frames (m,T,N,2): a start in [-0.7, 0.7]^2 and a velocity in [-0.12, 0.12]^2 per object,
    reflected at +-0.8"""
    p0 = torch.rand(m, 1, N, 2, generator=g, dtype=torch.float64) * 1.4 - 0.7
    v = torch.rand(m, 1, N, 2, generator=g, dtype=torch.float64) * 0.24 - 0.12
    p = p0 + v * torch.arange(T, dtype=torch.float64).view(1, T, 1, 1)
    return (0.8 - ((p + 0.8) % 3.2 - 1.6).abs()).numpy()


def model_decisions(N, regime, x, dtype):
    """The discrete decisions of the oracle's run in `dtype` on colour frames x (m,T,3,32,32): the matching indices (m,T,N) and the
    fix_supair hit masks (m,T,N) (helpers.state_chain on the oracle's own codes)"""
    c, _, params = _model_oracle(N, regime, dtype)
    m, T = x.shape[:2]
    with torch.no_grad():
        codes = O.encoder_forward(c, params, O.bw_transform(x.to(dtype)).flatten(0, 1))
        out = state_chain(c, codes.reshape(-1, 8), m, T, N, c.skip, c.debug_fix_supair, c.debug_match_objects)
    return out['idx'], out['hits']


_MODEL_ORACLES, _MODEL_INPUTS = {}, {}


def _model_oracle(N, regime, dtype):
    key = (N, regime, dtype)
    if key not in _MODEL_ORACLES:
        c, structs, params = oracle_setup(dtype, requires_grad=False, regime=regime, **model_cfg(N))
        _MODEL_ORACLES[key] = (c, structs, {k: v for k, v in params.items() if k.startswith('sup.encoder.')})
    return _MODEL_ORACLES[key]


def model_same_decisions(N, regime, x):
    """per sequence: the oracle's float32 run takes the matching and the fix_supair hits of its float64 run"""
    i64, h64 = model_decisions(N, regime, x, torch.float64)
    i32, h32 = model_decisions(N, regime, x, torch.float32)
    return (i64 == i32).flatten(1).all(1) & (h64 == h32).flatten(1).all(1)


def model_inputs(N, B, T, regime):
    """(x (B,T,3,32,32), eps as O.draw_eps) of a model case, float32 values in float64: the first B painted sequences of a seeded
    stream on which the oracle's float32 run takes its float64 run's decisions (model_same_decisions); drawn once, shared"""
    key = (N, B, T, regime)
    if key not in _MODEL_INPUTS:
        g = torch.Generator().manual_seed(810000 + 1000 * N + 10 * B + T + (500 if regime != 'analytic' else 0))
        seqs = _accept(g, B, lambda g_, m: (paint_discs(draw_tracks(g_, m, T, N), disc_radii(N)),),
                       lambda cand: model_same_decisions(N, regime, cand[0]), 'model N%d B%d T%d %s' % (N, B, T, regime))
        eps = O.draw_eps(B, N, T, generator=g, dtype=torch.float64)
        eps = {'latent': eps['latent'].float().double(), 'std': eps['std'].float().double(), 'steps': [e.float().double() for e in eps['steps']]}
        _MODEL_INPUTS[key] = (torch.stack([s[0] for s in seqs]), eps)
    return _MODEL_INPUTS[key]
