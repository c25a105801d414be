"""Record the reference's PPO update step by step for tests/test_ppo_update_cpu.py and tests/test_gpu_ppo_update.py:
tests/golden/g25_ppo_update.npz and g25_reference_fp32_gap.json.

    python tools/make_ppo_update_goldens.py --reference /path/to/the/reference/checkout

Nothing of the reference's text is copied: its classes are imported from the checkout (tools/make_ppo_goldens.py: load_reference),
run, and their inputs and outputs written down.  Data only.

Per shape s of (N, H, deep) = (3, 64, False), (6, 64, True), (1, 32, False), g24's shapes, policy and observations
(torch.manual_seed(100 + s), 64 real avoidance states), and per kind k of ('plain': max_grad_norm 40, no step clips; 'clip':
max_grad_norm 0.1, every step clips), case c = 2 s + k: a batch by g24's recipe from RandomState(seed) -- values and old
log-probabilities the policy's own plus noise of scale .05, returns N(-.5, .5), adv = returns - values --, then the reference's
PPOAgent.update with (E, M) = (2, 4), clip .1, coefficients .5 / .01, lr 2e-4, eps 1e-5 under torch.manual_seed(0): once on
policy.double(), once in float32.  The per-step quantities are taken while the reference runs: the permutations from torch.randperm,
each step's new values / log-probabilities / entropy from Policy.evaluate_actions, the gradient norm from clip_grad_norm_; the three
losses of a step are the reference's formulas on those outputs, and their averages are checked against what update() returns.

  s{s}_sd_<key>                       the policy before the update (float32)
  c{c}_obs, actions, returns, values, logp, adv, perm, hyper, seed
  c{c}_sd_<key>                       the float64 parameters after the update (unused in_between layers left out)
  c{c}_losses (8, 3), c{c}_gnorm (8,), c{c}_returned (3,)          float64
The json holds per case the float32-to-float64 gap (largest absolute parameter difference, and per step quantity the largest
difference over the steps) and the smallest decision margins of the float64 run over every row of every step: |ratio - (1 +- c)|,
||v - v_old| - c|, the difference of the two squared errors where the value is outside its clip range, |adv|, and
|norm - max_grad_norm| / max_grad_norm.  A case whose smallest margin is below 1e-5 is not written: the next seed (+ 6) is taken."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import make_ppo_goldens as g24  # noqa: E402

SHAPES = g24.SHAPES
KINDS = (('plain', 40.0), ('clip', 0.1))
E, M, CLIP, VALUE_COEF, ENTROPY_COEF, LR, EPS = 2, 4, .1, .5, .01, 2e-4, 1e-5
MIN_MARGIN = 1e-5


def batch(policy64, obs, case_actions, seed):
    """g24's recipe: -> returns, values, logp, adv (64, 1) float64"""
    with torch.no_grad():
        value, logp, _ = policy64.evaluate_actions(torch.from_numpy(obs).double(), torch.from_numpy(case_actions))
    rs = np.random.RandomState(seed)
    values = value + torch.from_numpy(rs.normal(scale=.05, size=(64, 1)))
    returns = torch.from_numpy(rs.normal(scale=.5, size=(64, 1))) - .5
    old = logp + torch.from_numpy(rs.normal(scale=.05, size=(64, 1)))
    return returns, values, old, returns - values


def traced_update(agents, policy, dtype, obs, actions, returns, values, logp, adv, max_grad_norm):
    """one reference update under torch.manual_seed(0) -> dict of the returned losses, the permutations and the per-step records"""
    agent = agents.PPOAgent(policy, CLIP, E, M, VALUE_COEF, ENTROPY_COEF, lr=LR, eps=EPS, max_grad_norm=max_grad_norm)
    rec = {'perm': [], 'eval': [], 'gnorm': []}
    randperm, clip_norm, evaluate = torch.randperm, torch.nn.utils.clip_grad_norm_, policy.evaluate_actions

    def traced_randperm(*a, **k):
        p = randperm(*a, **k)
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

    torch.randperm, torch.nn.utils.clip_grad_norm_, policy.evaluate_actions = traced_randperm, traced_clip, traced_evaluate
    try:
        torch.manual_seed(0)
        cast = lambda t: t.to(dtype)
        rec['returned'] = agent.update(torch.from_numpy(obs).to(dtype), torch.from_numpy(actions), cast(returns), cast(values), cast(logp), cast(adv))
    finally:
        torch.randperm, torch.nn.utils.clip_grad_norm_ = randperm, clip_norm
        del policy.evaluate_actions
    return rec


def step_quantities(rec, dtype, returns, values, logp, adv, max_grad_norm):
    """the reference's loss formulas on each step's recorded outputs, in the run's number format -> losses (E M, 3), and the margins"""
    n, mb = returns.shape[0], returns.shape[0] // M
    losses, margins = [], {'ratio': np.inf, 'value_clip': np.inf, 'value_max': np.inf, 'adv': np.inf, 'norm': np.inf}
    for at, (new_values, new_logp, entropy) in enumerate(rec['eval']):
        rows = torch.from_numpy(rec['perm'][at // M][(at % M) * mb:(at % M + 1) * mb])
        R, vo, lo, A = (t.to(dtype)[rows] for t in (returns, values, logp, adv))
        ratio = torch.exp(new_logp - lo)
        action_loss = -torch.min(ratio * A, torch.clamp(ratio, 1.0 - CLIP, 1.0 + CLIP) * A).mean()
        dv = new_values - vo
        l1, l2 = (new_values - R).pow(2), (vo + dv.clamp(-CLIP, CLIP) - R).pow(2)
        value_loss = 0.5 * torch.max(l1, l2).mean()
        losses.append([float(value_loss), float(action_loss), float(entropy)])
        margins['ratio'] = min(margins['ratio'], float(torch.min((ratio - (1 - CLIP)).abs(), (ratio - (1 + CLIP)).abs()).min()))
        margins['value_clip'] = min(margins['value_clip'], float((dv.abs() - CLIP).abs().min()))
        outside = dv.abs() > CLIP
        if bool(outside.any()):
            margins['value_max'] = min(margins['value_max'], float((l1 - l2)[outside].abs().min()))
        margins['adv'] = min(margins['adv'], float(A.abs().min()))
        margins['norm'] = min(margins['norm'], abs(rec['gnorm'][at] - max_grad_norm) / max_grad_norm)
    assert len(losses) == len(rec['gnorm']) == E * M and n >= M
    return np.array(losses), margins


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True)
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    args = ap.parse_args()
    rl_model, agents, _, _ = g24.load_reference(args.reference)
    G, J = {'shapes': np.int32(len(SHAPES)), 'EM': np.array([E, M], dtype=np.int32)}, {}
    for s, (N, H, deep) in enumerate(SHAPES):
        torch.manual_seed(100 + s)
        start = rl_model.Policy(4 * N, 9, hidden_size=H, base='control', use_deep_layers=deep)
        start_sd = {k: t.clone() for k, t in start.state_dict().items()}
        for k, t in start_sd.items():
            G['s%d_sd_%s' % (s, k)] = t.numpy().copy()
        obs = g24.observations(N)
        actions = np.random.RandomState(s).randint(9, size=(64, 1))
        for kind, (name, max_grad_norm) in enumerate(KINDS):
            c, seed = 2 * s + kind, 40 + s
            while True:
                runs = {}
                for tag, dt in (('64', torch.float64), ('32', torch.float32)):
                    policy = rl_model.Policy(4 * N, 9, hidden_size=H, base='control', use_deep_layers=deep)
                    policy.load_state_dict(start_sd)
                    policy = policy.to(dt)
                    if tag == '64':
                        returns, values, logp, adv = batch(policy, obs, actions, seed)
                    rec = traced_update(agents, policy, dt, obs, actions, returns, values, logp, adv, max_grad_norm)
                    rec['losses'], rec['margins'] = step_quantities(rec, dt, returns, values, logp, adv, max_grad_norm)
                    rec['sd'] = {k: t.detach().double().numpy().copy() for k, t in policy.state_dict().items()}
                    assert np.abs(rec['losses'].mean(0) - np.array(rec['returned'])).max() <= (1e-12 if tag == '64' else 1e-6)
                    runs[tag] = rec
                if min(runs['64']['margins'].values()) >= MIN_MARGIN:
                    break
                print('case %d: seed %d has a margin of %.3g, taking the next' % (c, seed, min(runs['64']['margins'].values())))
                seed += 6
            r64, r32 = runs['64'], runs['32']
            assert all(np.array_equal(a, b) for a, b in zip(r64['perm'], r32['perm']))
            clipped = [g > max_grad_norm for g in r64['gnorm']]
            assert all(clipped) if name == 'clip' else not any(clipped), (name, r64['gnorm'])
            pre = 'c%d_' % c
            G[pre + 'obs'], G[pre + 'actions'] = obs, actions[:, 0].astype(np.int64)
            for k, t in (('returns', returns), ('values', values), ('logp', logp), ('adv', adv)):
                G[pre + k] = t.numpy()[:, 0].copy()
            G[pre + 'perm'] = np.stack(r64['perm']).astype(np.int64)
            G[pre + 'hyper'] = np.array([CLIP, VALUE_COEF, ENTROPY_COEF, LR, EPS, max_grad_norm])
            G[pre + 'seed'] = np.int32(seed)
            G[pre + 'losses'], G[pre + 'gnorm'], G[pre + 'returned'] = r64['losses'], np.array(r64['gnorm']), np.array(r64['returned'])
            for k, t in r64['sd'].items():
                if 'in_between' in k and not deep:
                    assert np.array_equal(t, start_sd[k].double().numpy())
                    continue
                G[pre + 'sd_' + k] = t
            J['case%d' % c] = {
                'shape': [N, H, bool(deep)], 'kind': name, 'max_grad_norm': max_grad_norm, 'seed': seed, 'margins': r64['margins'],
                'gap': {'params': max(float(np.abs(r64['sd'][k] - r32['sd'][k]).max()) for k in r64['sd']),
                        'value_loss': float(np.abs(r64['losses'][:, 0] - r32['losses'][:, 0]).max()),
                        'action_loss': float(np.abs(r64['losses'][:, 1] - r32['losses'][:, 1]).max()),
                        'entropy': float(np.abs(r64['losses'][:, 2] - r32['losses'][:, 2]).max()),
                        'gnorm': float(np.abs(np.array(r64['gnorm']) - np.array(r32['gnorm'])).max())},
                'gnorm': [min(r64['gnorm']), max(r64['gnorm'])]}
    np.savez_compressed(os.path.join(args.out, 'g25_ppo_update.npz'), **G)
    with open(os.path.join(args.out, 'g25_reference_fp32_gap.json'), 'w') as fh:
        json.dump(J, fh, indent=1, sort_keys=True)
    print(json.dumps(J, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
