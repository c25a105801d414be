#!/usr/bin/env python
"""Write tests/golden/g23_mcts_env.npz: the reference's search on the true environment (model/mcts/mcts_env.py of a reference
checkout: class MCTS) run on the reference's own environments (model/envs/envs.py: BillardsEnv under AvoidanceTask), so that the host
and device searches of stove_amd.mcts.mcts_env can be held to it without the reference.

    python tools/make_mcts_env_goldens.py --reference /path/to/reference

Both files are loaded by path, with stand-ins for the third-party modules they import and this machine may lack.  The search module's
`np.random.randint` is replaced by a reader of a seeded table (runs, D): iteration i reads row i from column 0 on, which is the order
the batched searches use.  The environment is instrumented by a subclass that writes down every branch margin of simulate_physics.

Cases (N, D, runs): (3, 10, 60), (3, 3, 40), (6, 2, 12), (1, 4, 20).  Environment: BillardsEnv(n=N, hw=10, r=1., res=32, seed=s) under
AvoidanceTask(action_force=0.6), warmed up with 8 steps of action 0; table: RandomState(1000 + s).randint(9, size=(runs, D)).  Seeds s =
0, 1, .. are tried in order; taken is the first whose search has every branch margin either an exact tie (the ball clamped to that wall
and at rest on that axis) or >= 1e-6 over every simulated step, and whose smallest decision gap is >= 1e-9 (the gap: at every Descend
level, u_best minus the largest u among actions whose (Qsa, Nsa) differ from the best's).
Per case `c<i>_`: n, depth, runs, granularity, drift, hw, t, friction, action_force, seed; the root x, v (N, 2), r, m (N,); draws (runs,
D) int32; one row per edge (s, a) of the final tree, parents before children: keys (K, D) int8 -- the action digits of s then a, padded
with -1 --, nsa, qsa, ns (Ns of the node s + str(a); 0 where the reference has no entry), expanded (it has one); ns_root; action;
min_gap; low (the smallest expansion value: < -1 means a rollout collected more than one collision)."""
import argparse
import importlib
import importlib.util
import os
import sys
import types

import numpy as np

A, WARMUP, MARGIN, MIN_GAP = 9, 8, 1e-6, 1e-9
CASES = ((3, 10, 60), (3, 3, 40), (6, 2, 12), (1, 4, 20))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_reference(path):
    """-> (the reference's envs module, its mcts_env module); modules they import and this machine lacks become empty stand-ins"""
    for name, attrs in (('spriteworld', ()), ('spriteworld.renderers', ()), ('spriteworld.sprite', ('Sprite',)), ('imageio', ()),
                        ('tqdm', ('tqdm',)), ('model', ()), ('model.envs', ())):
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
    mcts = _load(os.path.join(path, 'model', 'mcts', 'mcts_env.py'), 'reference_mcts_env')
    return envs, mcts


class Table:
    """stands in for the search module's `np`: everything is numpy's, except random.randint, which reads row `row` of the table"""

    def __init__(self, table):
        self.table, self.row, self.col = table, 0, 0
        self.random = types.SimpleNamespace(randint=self._next)

    def start(self, row):
        self.row, self.col = row, 0

    def _next(self, high):
        assert high == A
        a = int(self.table[self.row, self.col])
        self.col += 1
        return a

    def __getattr__(self, name):
        return getattr(np, name)


def recording(envs):
    """a subclass of the reference's BillardsEnv whose simulate_physics is the base class's, statement for statement, with every branch
    margin written down as (margin, is an exact tie that any arithmetic reproduces)"""

    class Recording(envs.BillardsEnv):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.margins = []

        def simulate_physics(self, actions):
            v = self.v.copy()
            dt = self.eps * self.t
            for i in range(self.n):
                for ax in range(2):
                    nxt = self.x[i, ax] + v[i, ax] * dt
                    ri = float(np.ravel(self.r[i])[0])
                    for wall in (ri, self.hw - ri):
                        self.margins.append((abs(nxt - wall), bool(self.x[i, ax] == wall and v[i, ax] == 0)))
                    if nxt < ri:
                        self.x[i, ax] = ri
                        v[i, ax] = -v[i, ax]
                    elif nxt > self.hw - ri:
                        self.x[i, ax] = self.hw - ri
                        v[i, ax] = -v[i, ax]
            if self.drift:
                return v
            for i in range(self.n):
                for j in range(i):
                    gap = envs.norm((self.x[i] + v[i] * self.t * self.eps) - (self.x[j] + v[j] * self.t * self.eps))
                    self.margins.append((abs(float(np.ravel(gap)[0]) - float(np.ravel(self.r[i] + self.r[j])[0])), False))
                    if gap < self.r[i] + self.r[j]:
                        controlled = actions and j == 0
                        if controlled:
                            self.collisions = 1
                        w = self.x[i] - self.x[j]
                        w = w / envs.norm(w)
                        v_i, v_j = np.dot(w.transpose(), v[i]), np.dot(w.transpose(), v[j])
                        if controlled:
                            v_j = 0
                        m1, m2 = self.m[i], self.m[j]
                        new_v_j = (2 * m1 * v_i + v_j * (m2 - m1)) / (m1 + m2)
                        new_v_i = new_v_j + (v_j - v_i)
                        v[i] += w * (new_v_i - v_i)
                        v[j] += w * (new_v_j - v_j)
                        if controlled:
                            v[j] = 0
            return v

    return Recording


def decision_gap(tree):
    """the Descend levels the next iteration will pass on the tree as it stands -> smallest u_best - u_a among a whose (Qsa, Nsa)
    differ from the best's"""
    s, gap = 'r', float('inf')
    while (s, 0) in tree.Qsa and len(s) + 1 != tree.max_rollout:
        u = [tree.Qsa[(s, a)] + tree.c * np.sqrt(np.log(tree.Ns[s]) / (1 + tree.Nsa[(s, a)])) for a in range(A)]
        best = int(np.argmax(u))
        for a in range(A):
            if (tree.Qsa[(s, a)], tree.Nsa[(s, a)]) != (tree.Qsa[(s, best)], tree.Nsa[(s, best)]):
                gap = min(gap, u[best] - u[a])
        s = s + str(best)
    return gap


def run(envs, mcts, N, D, runs, seed):
    env = recording(envs)(n=N, hw=10, r=1., res=32, seed=seed)
    task = envs.AvoidanceTask(env, action_force=0.6)
    for _ in range(WARMUP):
        task.step(0)
    table = np.random.RandomState(1000 + seed).randint(A, size=(runs, D)).astype(np.int32)
    reader = Table(table)
    mcts.np = reader
    try:
        tree = mcts.MCTS(task, max_rollout=D)
        root = dict(x=np.array(env.x, dtype=np.float64), v=np.array(env.v, dtype=np.float64), r=np.ravel(env.r).astype(np.float64),
                    m=np.ravel(env.m).astype(np.float64))
        gap, low = float('inf'), 0.0
        for i in range(runs):
            gap = min(gap, decision_gap(tree))
            reader.start(i)
            low = min(low, float(tree.select(tree.env, 'r')))
            tree.env_reset()
    finally:
        mcts.np = np
    edges = sorted((k for k in tree.Qsa if isinstance(k, tuple)), key=lambda k: (len(k[0]), k[0], k[1]))
    keys = np.full((len(edges), D), -1, dtype=np.int8)
    for i, (s, a) in enumerate(edges):
        d = [int(ch) for ch in s[1:]] + [a]
        keys[i, :len(d)] = d
    action = int(np.argmax([tree.Nsa[('r', a)] for a in range(A)]))
    margins = [mg for mg, tie in env.margins if not tie]
    rec = dict(root, n=np.int64(N), depth=np.int64(D), runs=np.int64(runs), granularity=np.int64(env.internal_steps), drift=np.int64(env.drift),
               hw=np.float64(env.hw), t=np.float64(env.t), friction=np.float64(env.fric_coeff), action_force=np.float64(task.action_force),
               seed=np.int64(seed), draws=table, keys=keys, nsa=np.array([tree.Nsa[k] for k in edges], dtype=np.int64),
               qsa=np.array([tree.Qsa[k] for k in edges], dtype=np.float64),
               ns=np.array([tree.Ns.get(s + str(a), 0) for s, a in edges], dtype=np.int64),
               expanded=np.array([(s + str(a), 0) in tree.Qsa for s, a in edges], dtype=bool), ns_root=np.int64(tree.Ns['r']),
               action=np.int64(action), min_gap=np.float64(gap), low=np.float64(low))
    return rec, (min(margins) if margins else float('inf')), all(mg == 0.0 for mg, tie in env.margins if tie)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of a reference checkout (holds model/mcts/mcts_env.py and model/envs/envs.py)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'g23_mcts_env.npz'))
    args = ap.parse_args()
    envs, mcts = load_reference(args.reference)
    out = {'cases': np.int64(len(CASES))}
    for c, (N, D, runs) in enumerate(CASES):
        skipped = []
        for seed in range(1000):
            rec, margin, ties = run(envs, mcts, N, D, runs, seed)
            if margin >= MARGIN and ties and rec['min_gap'] >= MIN_GAP:
                break
            skipped.append('seed %d: %s' % (seed, 'a branch margin of %.3g' % margin if margin < MARGIN or not ties
                                            else 'a decision gap of %.3g' % rec['min_gap']))
        else:
            raise RuntimeError('no seed below 1000 serves N = %d, D = %d' % (N, D))
        print('N = %d, D = %d, runs = %d: seed %d after %d skipped (%s); smallest margin %.3g, decision gap %.3g, %d edges, action %d, '
              'lowest value %g' % (N, D, runs, seed, len(skipped), '; '.join(skipped) or 'none', margin, rec['min_gap'], len(rec['nsa']),
                                   rec['action'], rec['low']))
        out.update({'c%d_%s' % (c, k): val for k, val in rec.items()})
    np.savez_compressed(args.out, **out)
    print('wrote', args.out, os.path.getsize(args.out), 'bytes')


if __name__ == '__main__':
    main()
