"""Record the reference's PPO arm for tests/test_ppo_cpu.py: tests/golden/g24_ppo.npz and g24_reference_fp32_gap.json.

    python tools/make_ppo_goldens.py --reference /path/to/the/reference/checkout

The reference's model/rl/rl_model.py and agents.py need only torch; runners.py (for Runner._calculate_returns) imports tensorboardX,
which becomes an empty stand-in when this machine lacks it, as do the modules its envs.py imports for rendering sprites.  Nothing of the
reference's text is copied: its classes are imported from the checkout, run, and their inputs and outputs written down.

Per case c of (N, H, deep) = (3, 64, False), (6, 64, True), (1, 32, False):
  c{c}_sd_<key>            the state_dict of Policy(4N, 9, hidden_size=H, base='control', use_deep_layers=deep) under torch.manual_seed(100 + c)
  c{c}_obs (64, 4N) f32    observations of real avoidance states (16 seeds, 4 steps apart); c{c}_actions (64,) the actions evaluated
  c{c}_value64, logits64, eval_value64, eval_logp64, eval_entropy64    the reference's outputs on policy.double(), and ..32 in float32
  c{c}_upd_*               a fixed batch (returns, values, logp, adv) and c{c}_upd_sd_<key>, the parameters after ONE PPOAgent.update in
                           float64 (clip .1, ppo_epoch 2, num_mini_batch 4, coefficients .5 / .01, lr 2e-4, eps 1e-5, max_grad_norm 40)
                           under torch.manual_seed(0), with its three returned losses
  ret_*                    Runner._calculate_returns on a fixed float32 reward table (discount .95)
  reset_*                  BillardsEnv(n, seed) under AvoidanceTask: x, v after each of three `reset()` + `step(0)`, for (n, seed) pairs
The json holds, per case, the largest deviation of the reference's own float32 outputs from its float64 outputs."""
import argparse
import importlib
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((3, 64, False), (6, 64, True), (1, 32, False))
RESETS = ((3, 0), (3, 7), (6, 1), (1, 2))


def _load(path, name, package=None):
    spec = importlib.util.spec_from_file_location(name, path, submodule_search_locations=None)
    mod = importlib.util.module_from_spec(spec)
    if package:
        mod.__package__ = package
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference(path):
    """-> (rl_model, agents, runners, envs) of the checkout; modules they import and this machine lacks become empty stand-ins"""
    for name, attrs in (('spriteworld', ()), ('spriteworld.renderers', ()), ('spriteworld.sprite', ('Sprite',)), ('imageio', ()),
                        ('tqdm', ('tqdm',)), ('tensorboardX', ('SummaryWriter',))):
        try:
            importlib.import_module(name)
        except ImportError:
            mod = types.ModuleType(name)
            for a in attrs:
                setattr(mod, a, object)
            sys.modules[name] = mod
    if not hasattr(sys.modules['spriteworld'], 'renderers'):
        sys.modules['spriteworld'].renderers = sys.modules['spriteworld.renderers']
    envs = _load(os.path.join(path, 'model', 'envs', 'envs.py'), 'reference_envs')
    # runners.py imports `.agents`, `.rl_model` and `model.envs.envs`: a package of the checkout's rl directory, and its envs under that name
    pkg = types.ModuleType('reference_rl')
    pkg.__path__ = [os.path.join(path, 'model', 'rl')]
    sys.modules['reference_rl'] = pkg
    for name in ('model', 'model.envs'):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules['model.envs.envs'] = envs
    mods = [_load(os.path.join(path, 'model', 'rl', f + '.py'), 'reference_rl.' + f, 'reference_rl') for f in ('rl_model', 'agents', 'runners')]
    return mods[0], mods[1], mods[2], envs


def observations(N):
    """64 observations of real avoidance states: 16 seeds, every fourth of 16 steps under a cycling action"""
    sys.path.insert(0, ROOT)
    from stove_amd.envs.batched import BatchedAvoidance
    b = BatchedAvoidance(range(16), n=N, granularity=2, action_force=.3)
    rows = []
    for step in range(16):
        b.step((np.arange(16) + step) % 9, render=False)
        if step % 4 == 3:
            rows.append(b.state().reshape(16, -1).astype(np.float32))
    return np.concatenate(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True)
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    args = ap.parse_args()
    rl_model, agents, runners, envs = load_reference(args.reference)
    G, gap = {'cases': np.int32(len(SHAPES))}, {}
    for c, (N, H, deep) in enumerate(SHAPES):
        pre = 'c%d_' % c
        torch.manual_seed(100 + c)
        policy = rl_model.Policy(4 * N, 9, hidden_size=H, base='control', use_deep_layers=deep)
        for k, ten in policy.state_dict().items():
            G[pre + 'sd_' + k] = ten.numpy().copy()
        obs = observations(N)
        actions = np.random.RandomState(c).randint(9, size=(64, 1))
        G[pre + 'obs'], G[pre + 'actions'] = obs, actions[:, 0].astype(np.int64)
        res = {}
        for tag, dt in (('32', torch.float32), ('64', torch.float64)):
            p = policy.to(dt)
            o = torch.from_numpy(obs).to(dt)
            with torch.no_grad():
                value, dist = p.head(p.base(o))
                ev, elp, ent = p.evaluate_actions(o, torch.from_numpy(actions))
            res[tag] = {'value': value, 'logits': dist.logits, 'eval_value': ev, 'eval_logp': elp, 'eval_entropy': ent}
            for k, ten in res[tag].items():
                G[pre + k + tag] = ten.numpy().copy()
        gap['case%d' % c] = {'shape': [N, H, bool(deep)],
                             **{k: float((res['32'][k].double() - res['64'][k]).abs().max()) for k in ('value', 'logits', 'eval_logp')}}
        # ---- one update in float64 (policy is float64 after the loop above)
        rs = np.random.RandomState(40 + c)
        values = res['64']['eval_value'] + torch.from_numpy(rs.normal(scale=.05, size=(64, 1)))
        returns = torch.from_numpy(rs.normal(scale=.5, size=(64, 1))) - .5
        logp = res['64']['eval_logp'] + torch.from_numpy(rs.normal(scale=.05, size=(64, 1)))
        adv = returns - values
        for k, ten in (('returns', returns), ('values', values), ('logp', logp), ('adv', adv)):
            G[pre + 'upd_' + k] = ten.numpy().copy()
        agent = agents.PPOAgent(policy, .1, 2, 4, .5, .01, lr=2e-4, eps=1e-5, max_grad_norm=40)
        torch.manual_seed(0)
        losses = agent.update(torch.from_numpy(obs).double(), torch.from_numpy(actions), returns, values, logp, adv)
        G[pre + 'upd_losses'] = np.array(losses, dtype=np.float64)
        for k, ten in policy.state_dict().items():
            G[pre + 'upd_sd_' + k] = ten.detach().numpy().copy()
    # ---- _calculate_returns
    rs = np.random.RandomState(3)
    rewards = torch.from_numpy(-(rs.random_sample((4, 10, 1)) < .3).astype(np.float32))
    next_value = torch.from_numpy(rs.normal(size=(4, 1)).astype(np.float32))
    runner = object.__new__(runners.Runner)
    runner.device, runner.discount = 'cpu', 0.95
    G['ret_rewards'], G['ret_next'] = rewards.numpy(), next_value.numpy()
    G['ret_out'] = runner._calculate_returns(next_value, rewards, torch.zeros(4, 10, 1)).numpy().copy()
    # ---- reset
    for k, (n, seed) in enumerate(RESETS):
        env = envs.BillardsEnv(n=n, seed=seed)
        task = envs.AvoidanceTask(env)
        xs, vs = [], []
        for _ in range(3):
            env.reset()
            task.step(0)
            xs.append(env.x.copy())
            vs.append(env.v.copy())
        G['reset%d_n' % k], G['reset%d_seed' % k] = np.int32(n), np.int32(seed)
        G['reset%d_x' % k], G['reset%d_v' % k] = np.stack(xs), np.stack(vs)
    G['resets'] = np.int32(len(RESETS))
    np.savez_compressed(os.path.join(args.out, 'g24_ppo.npz'), **G)
    with open(os.path.join(args.out, 'g24_reference_fp32_gap.json'), 'w') as fh:
        json.dump(gap, fh, indent=1, sort_keys=True)
    print(json.dumps(gap, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
