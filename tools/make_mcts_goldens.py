#!/usr/bin/env python
"""Write tests/golden/g21_mcts_tree.npz: the reference's MCTS class (model/mcts/mcts_stove.py of a reference checkout) driven with
seeded synthetic rewards, so that the host tree of stove_amd.mcts can be replayed against it without the reference.

    python tools/make_mcts_goldens.py --reference /path/to/reference

Per rollout depth D in (3, 10), with A = 9 actions and 60 iterations: the inputs of every backpropagate call (rs (A,1,1), r_rollout
(A,2D,1), new_zs (A,1,1,2), float32), the key selected at every iteration, every key's final Nsa / Qsa / Ns, the chosen action, the
seed, and the smallest gap between the best and the second-best UCT value over all decisions of the run.  Seeds are tried in order
until that gap is at least 1e-4: float32-against-float64 rounding of a Qsa (1e-7) can then not flip a decision.
Keys are stored as their action digits, padded with -1 ('r31' -> [3, 1, -1, ...])."""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

A, ITERS, DEPTHS, MIN_GAP = 9, 60, (3, 10), 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_reference(path):
    """the reference's mcts_stove module; third-party modules it imports and this machine lacks become empty stand-ins"""
    for name, attrs in (('model', ()), ('model.envs', ()), ('imageio', ()), ('tqdm', ('tqdm',)), ('multiprocess', ('Pool',))):
        try:
            importlib.import_module(name)
        except ImportError:
            mod = types.ModuleType(name)
            for a in attrs:
                setattr(mod, a, None)
            sys.modules[name] = mod
    spec = importlib.util.spec_from_file_location('reference_mcts_stove', os.path.join(path, 'model', 'mcts', 'mcts_stove.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def decision_gap(tree):
    """the walk of the reference's select on the tree as it stands -> smallest (best - second best) over [cur_best, u_0 .. u_{A-1}]
    of every level it passes"""
    s, cur_best, best_act, gap = 'r', -float('inf'), 0, float('inf')
    while (s + '0') in tree.Qsa and len(s) != tree.max_rollout:
        u = [tree.Qsa[s + str(a)] + tree.c * np.sqrt(np.log(tree.Ns[s]) / (1 + tree.Nsa[s + str(a)])) for a in range(tree.actions)]
        top = sorted([cur_best] + u)
        if np.isfinite(top[-1] - top[-2]):
            gap = min(gap, top[-1] - top[-2])
        for a, v in enumerate(u):
            if v > cur_best:
                cur_best, best_act = v, a
        s = s + str(best_act)
    return gap


def digits(keys, width):
    out = np.full((len(keys), width), -1, dtype=np.int64)
    for i, k in enumerate(keys):
        out[i, :len(k) - 1] = [int(c) for c in k[1:]]
    return out


def run(ref, D, seed):
    g = torch.Generator().manual_seed(seed)
    rs = torch.rand(ITERS, A, 1, 1, generator=g)
    rr = torch.rand(ITERS, A, 2 * D, 1, generator=g)
    zs = torch.rand(ITERS, A, 1, 1, 2, generator=g)
    z0 = torch.rand(1, 1, 2, generator=g)
    tree = ref.MCTS(torch.zeros(1, 1, 3), z0, action_space=A, max_rollout_depth=D)
    selected, gap = [], float('inf')
    for i in range(ITERS):
        gap = min(gap, decision_gap(tree))
        s, _ = tree.select('r', tree.Zstate['r'])
        selected.append(s)
        tree.backpropagate(zs[i], rs[i], rr[i], s)
    keys = sorted(tree.Qsa.keys(), key=lambda k: (len(k), k))
    action = int(np.argmax([tree.Nsa['r' + str(a)] for a in range(A)]))
    return dict(rs=rs.numpy(), rr=rr.numpy(), zs=zs.numpy(), z0=z0.numpy(), sel=digits(selected, D + 1), keys=digits(keys, D + 1),
                nsa=np.array([tree.Nsa[k] for k in keys], dtype=np.int64), qsa=np.array([tree.Qsa[k] for k in keys], dtype=np.float64),
                ns=np.array([tree.Ns[k] for k in keys], dtype=np.int64), action=np.int64(action), seed=np.int64(seed), gap=np.float64(gap))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of a reference checkout (holds model/mcts/mcts_stove.py)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'g21_mcts_tree.npz'))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    ref = load_reference(args.reference)
    out = {'actions': np.int64(A), 'iters': np.int64(ITERS), 'depths': np.array(DEPTHS, dtype=np.int64)}
    for D in DEPTHS:
        for seed in range(1000):
            rec = run(ref, D, seed)
            if rec['gap'] >= MIN_GAP:
                break
        else:
            raise RuntimeError('no seed below 1000 keeps every decision %g apart at depth %d' % (MIN_GAP, D))
        print('depth %d: seed %d, smallest decision gap %.3g, %d keys, action %d' % (D, seed, rec['gap'], len(rec['nsa']), rec['action']))
        out.update({'%s_d%d' % (k, D): v for k, v in rec.items()})
    np.savez_compressed(args.out, **out)
    print('wrote', args.out, os.path.getsize(args.out), 'bytes')


if __name__ == '__main__':
    main()
