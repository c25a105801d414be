"""Shared cases of the tests of the one-launch PPO update (tests/test_ppo_update_cpu.py, tests/test_gpu_ppo_update.py): the reference's
recorded updates (tests/golden/g25_ppo_update.npz, tools/make_ppo_update_goldens.py), the seeded edge shapes with their float64 and
float32 torch runs of this project's PPOAgent.update (computed once per shape, never modified), and the comparison against the bar:
4 x the float32-to-float64 gap of the same update, per case and per quantity, never taken from the code under test."""
import functools
import json
import os

import numpy as np
import torch

from stove_amd.envs.batched import BatchedAvoidance
from stove_amd.rl.agents import PPOAgent
from stove_amd.rl.rl_model import Policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_SHAPES = ((3, 64, False), (6, 64, True), (1, 32, False))
CASES = tuple(range(6))                     # case c: shape c // 2, kind 'plain' (max_grad_norm 40) / 'clip' (0.1)
QUANTITIES = ('params', 'value_loss', 'action_loss', 'entropy', 'gnorm')
MIN_MARGIN, FACTOR = 1e-5, 4
HYPER = ('clip', 'value_coef', 'entropy_coef', 'lr', 'eps', 'max_grad_norm')


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'g25_ppo_update.npz'))


@functools.lru_cache(maxsize=None)
def gaps():
    with open(os.path.join(ROOT, 'tests', 'golden', 'g25_reference_fp32_gap.json')) as fh:
        return json.load(fh)


def policy_of(shape, state, dtype=torch.float32):
    N, H, deep = shape
    p = Policy(4 * N, 9, hidden_size=H, base='control', use_deep_layers=deep)
    p.load_state_dict(state)
    return p.to(dtype)


def golden_start(c, dtype=torch.float32):
    """the policy before the update of golden case c"""
    G, pre = golden(), 's%d_sd_' % (c // 2)
    return policy_of(GOLDEN_SHAPES[c // 2], {k[len(pre):]: torch.from_numpy(G[k]) for k in G.files if k.startswith(pre)}, dtype)


def golden_after(c):
    """the recorded float64 parameters after the update, by state_dict key (the layers a shallow policy never uses left out)"""
    G, pre = golden(), 'c%d_sd_' % c
    return {k[len(pre):]: G[k] for k in G.files if k.startswith(pre)}


def golden_batch(c):
    """-> dict of obs (n, 4N) f32, actions (n,) i64, returns, values, logp, adv (n,) f64, perm (E, n) i64, M, the hyperparameters"""
    G, pre = golden(), 'c%d_' % c
    out = {k: G[pre + k] for k in ('obs', 'actions', 'returns', 'values', 'logp', 'adv', 'perm')}
    out['M'] = int(G['EM'][1])
    out.update(zip(HYPER, (float(x) for x in G[pre + 'hyper'])))
    return out


# ------------------------------------------------------------------------------------------------ this project's torch update, traced
def traced_update(policy, batch, dtype, perm=None, seed=0, use_clipped_value_loss=True):
    """PPOAgent.update (torch autograd) on `policy` in `dtype` with its per-step quantities taken while it runs: the permutations (perm
    given: those are used instead of torch.randperm under `seed`), each step's losses by the update's own formulas on the outputs of
    evaluate_actions, the gradient norm clip_grad_norm_ returns.  -> dict perm (E, n), losses (E M, 3), gnorm (E M,), sd, margins"""
    E = len(perm) if perm is not None else batch['E']
    M, c = batch['M'], batch['clip']
    agent = PPOAgent(policy, c, E, M, batch['value_coef'], batch['entropy_coef'], lr=batch['lr'], eps=batch['eps'],
                     max_grad_norm=batch['max_grad_norm'], use_clipped_value_loss=use_clipped_value_loss)
    rec = {'perm': [], 'eval': [], 'gnorm': []}
    randperm, clip_norm, evaluate = torch.randperm, torch.nn.utils.clip_grad_norm_, policy.evaluate_actions

    def traced_randperm(n):
        p = torch.from_numpy(np.asarray(perm[len(rec['perm'])]).astype(np.int64)) if perm is not None else randperm(n)
        rec['perm'].append(p.numpy().copy())
        return p

    def traced_clip(*a, **k):
        total = clip_norm(*a, **k)
        rec['gnorm'].append(float(total))
        return total

    def traced_evaluate(o, a):
        out = evaluate(o, a)
        rec['eval'].append(tuple(t.detach().clone() for t in out))
        return out

    col = lambda k: torch.from_numpy(np.asarray(batch[k])).to(dtype).reshape(-1, 1)
    returns, values, logp, adv = col('returns'), col('values'), col('logp'), col('adv')
    state = torch.get_rng_state()
    torch.randperm, torch.nn.utils.clip_grad_norm_, policy.evaluate_actions = traced_randperm, traced_clip, traced_evaluate
    try:
        torch.manual_seed(seed)
        returned = agent.update(torch.from_numpy(batch['obs']).to(dtype), torch.from_numpy(np.asarray(batch['actions'])).long().reshape(-1, 1),
                                returns, values, logp, adv)
    finally:
        torch.randperm, torch.nn.utils.clip_grad_norm_ = randperm, clip_norm
        del policy.evaluate_actions
        torch.set_rng_state(state)
    n = returns.shape[0]
    mb = n // M
    losses, margins = [], {'ratio': np.inf, 'value_clip': np.inf, 'value_max': np.inf, 'adv': np.inf, 'norm': np.inf}
    for at, (new_values, new_logp, entropy) in enumerate(rec['eval']):
        rows = torch.from_numpy(rec['perm'][at // M][(at % M) * mb:(at % M + 1) * mb])
        R, vo, lo, A = returns[rows], values[rows], logp[rows], adv[rows]
        ratio = torch.exp(new_logp - lo)
        action_loss = -torch.min(ratio * A, torch.clamp(ratio, 1.0 - c, 1.0 + c) * A).mean()
        dv = new_values - vo
        l1, l2 = (new_values - R).pow(2), (vo + dv.clamp(-c, c) - R).pow(2)
        losses.append([float(0.5 * torch.max(l1, l2).mean()), float(action_loss), float(entropy)])
        margins['ratio'] = min(margins['ratio'], float(torch.min((ratio - (1 - c)).abs(), (ratio - (1 + c)).abs()).min()))
        margins['value_clip'] = min(margins['value_clip'], float((dv.abs() - c).abs().min()))
        if bool((dv.abs() > c).any()):
            margins['value_max'] = min(margins['value_max'], float((l1 - l2)[dv.abs() > c].abs().min()))
        margins['adv'] = min(margins['adv'], float(A.abs().min()))
        margins['norm'] = min(margins['norm'], abs(rec['gnorm'][at] - batch['max_grad_norm']) / batch['max_grad_norm'])
    losses = np.array(losses, dtype=np.float64).reshape(len(rec['eval']), 3)
    assert len(losses) == E * M and np.allclose(losses.mean(0), returned, rtol=0, atol=1e-12 if dtype == torch.float64 else 1e-5)
    return {'perm': np.stack(rec['perm']), 'losses': losses, 'gnorm': np.array(rec['gnorm']), 'margins': margins, 'returned': returned,
            'sd': {k: t.detach().double().numpy().copy() for k, t in policy.state_dict().items()}}


# ------------------------------------------------------------------------------------------------ the edge shapes (not in the fixture)
# name -> (N, H, deep, n, E, M, max_grad_norm)
EDGES = {
    'n6_h40': (6, 40, False, 64, 2, 4, 40.0),                   # H no multiple of the wave or of 32
    'n6_h128_deep': (6, 128, True, 64, 2, 4, 40.0),             # the image that does not fit LDS
    'n1_h32_clip': (1, 32, False, 64, 2, 4, 0.1),               # one object, every step clips
    'n70_m4': (3, 64, False, 70, 2, 4, 40.0),                   # mb = 17: two rows dropped per epoch, a second tile of one row
    'mb1': (3, 64, False, 8, 1, 8, 40.0),                       # one row per step
    'm1': (3, 64, True, 64, 2, 1, 40.0),                        # one step per epoch, four full tiles
    'e1': (3, 64, False, 64, 1, 4, 40.0),
}


def observations(N, n):
    """n observations of real avoidance states: 16 seeds, every fourth step under a cycling action (the generator's, for any n)"""
    b = BatchedAvoidance(range(16), n=N, granularity=2, action_force=.3)
    rows, step = [], 0
    while 16 * len(rows) < n:
        b.step((np.arange(16) + step) % 9, render=False)
        if step % 4 == 3:
            rows.append(b.state().reshape(16, -1).astype(np.float32))
        step += 1
    return np.concatenate(rows)[:n].copy()


@functools.lru_cache(maxsize=None)
def edge(name):
    """-> (shape, start state_dict, batch dict with perm, the float64 run, the gap per quantity, the seed taken, seeds skipped); read only.
    The batch by the generator's recipe from RandomState(seed), seeds from 40 on; a seed whose float64 margins fall below 1e-5 is passed
    over."""
    N, H, deep, n, E, M, max_grad_norm = EDGES[name]
    state = torch.get_rng_state()
    torch.manual_seed(100 + sum(map(ord, name)))
    start = {k: t.clone() for k, t in Policy(4 * N, 9, hidden_size=H, base='control', use_deep_layers=deep).state_dict().items()}
    torch.set_rng_state(state)
    shape = (N, H, deep)
    obs = observations(N, n)
    actions = np.random.RandomState(sum(map(ord, name))).randint(9, size=n)
    skipped = 0
    for seed in range(40, 44):
        p64 = policy_of(shape, start, torch.float64)
        with torch.no_grad():
            value, logp, _ = p64.evaluate_actions(torch.from_numpy(obs).double(), torch.from_numpy(actions).reshape(-1, 1))
        rs = np.random.RandomState(seed)
        values = value.numpy()[:, 0] + rs.normal(scale=.05, size=n)
        returns = rs.normal(scale=.5, size=n) - .5
        old = logp.numpy()[:, 0] + rs.normal(scale=.05, size=n)
        batch = {'obs': obs, 'actions': actions, 'returns': returns, 'values': values, 'logp': old, 'adv': returns - values, 'M': M, 'E': E,
                 'clip': .1, 'value_coef': .5, 'entropy_coef': .01, 'lr': 2e-4, 'eps': 1e-5, 'max_grad_norm': max_grad_norm}
        r64 = traced_update(p64, batch, torch.float64)
        if min(r64['margins'].values()) >= MIN_MARGIN:
            break
        skipped += 1
    r32 = traced_update(policy_of(shape, start), batch, torch.float32, perm=r64['perm'])
    batch['perm'] = r64['perm']
    return shape, start, batch, r64, gap_of(r64, r32), seed, skipped


def gap_of(r64, r32):
    return {'params': max(float(np.abs(r64['sd'][k] - r32['sd'][k]).max()) for k in r64['sd']),
            'value_loss': float(np.abs(r64['losses'][:, 0] - r32['losses'][:, 0]).max()),
            'action_loss': float(np.abs(r64['losses'][:, 1] - r32['losses'][:, 1]).max()),
            'entropy': float(np.abs(r64['losses'][:, 2] - r32['losses'][:, 2]).max()),
            'gnorm': float(np.abs(r64['gnorm'] - r32['gnorm']).max())}


# ------------------------------------------------------------------------------------------------ the comparison
def distances(shape, image, losses, gnorm, want_sd, want_losses, want_gnorm):
    """the largest absolute distance per quantity of an update's results (the float32 image after it, losses (steps, 3), gnorm (steps,))
    from the float64 ones (a state_dict's arrays; keys it lacks are not compared)"""
    p = Policy(4 * shape[0], 9, hidden_size=shape[1], base='control', use_deep_layers=shape[2])
    p.load_flat_params(torch.from_numpy(np.array(image, dtype=np.float32)))
    sd = p.state_dict()
    losses, gnorm = np.asarray(losses, dtype=np.float64), np.asarray(gnorm, dtype=np.float64)
    used = [k for k in want_sd if shape[2] or 'in_between' not in k]
    return {'params': max(float(np.abs(sd[k].double().numpy() - want_sd[k]).max()) for k in used),
            'value_loss': float(np.abs(losses[:, 0] - want_losses[:, 0]).max()), 'action_loss': float(np.abs(losses[:, 1] - want_losses[:, 1]).max()),
            'entropy': float(np.abs(losses[:, 2] - want_losses[:, 2]).max()), 'gnorm': float(np.abs(gnorm - want_gnorm).max())}


def hold_to_the_bar(label, got, gap):
    """print every distance beside its bar, then assert them all"""
    for q in QUANTITIES:
        print(f'{label}: {q} off by {got[q]:.3g} (bar {FACTOR * gap[q]:.3g}, {got[q] / gap[q] if gap[q] else float("inf"):.2f} x the gap)')
    missed = [q for q in QUANTITIES if not got[q] <= FACTOR * gap[q]]
    assert not missed, (label, {q: (got[q], FACTOR * gap[q]) for q in missed})


def kernel_inputs(policy, batch):
    """numpy arrays in the kernel's formats: image, obs f32, actions i32, returns, values, logp, adv f32, perm i32"""
    f32 = lambda k: np.ascontiguousarray(batch[k], dtype=np.float32)
    return {'image': policy.flat_params().numpy().copy(), 'obs': f32('obs'), 'actions': np.ascontiguousarray(batch['actions'], dtype=np.int32),
            'returns': f32('returns'), 'values': f32('values'), 'logp': f32('logp'), 'adv': f32('adv'),
            'perm': np.ascontiguousarray(batch['perm'], dtype=np.int32)}
