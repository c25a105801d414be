"""Tree search on the TRUE environment (reference model/mcts/mcts_env.py; scripts/run_mcts.py: main_mcts_env): the upper baseline the
learned model's planner (mcts_stove.py) is judged against.

`MCTS` is the reference's class surface on one AvoidanceTask -- a recursion that draws np.random.randint(A) one at a time.  `EnvForest`
is the same search for T trees at once in numpy, and the specification of the device search (csrc/env_search.h, stove_env_search):

A tree has A = 9 actions, c = 1 and depth D = max_rollout >= 2.  A node is its action string s ('r' the root, len('r') = 1).  One
iteration starts at the root with the environment at the root state and walks down:
  Expand    s has no edges yet (len(s) < D always holds there): Ns[s] = 0, every Qsa[(s, .)] = -1 and Nsa[(s, .)] = 0; the environment
            is stepped with a drawn action a (reward r), then D - len(s) more times with drawn actions; value = r + the plain sum of
            those rewards; the edge is (s, a) and its Q is updated.
  Descend   s has edges and len(s) + 1 != D: the first-index argmax of Qsa + c sqrt(log(Ns[s]) / (1 + Nsa)) with strict >, from -inf
            FRESH at every level (mcts_stove.py carries its running best across levels; this search does not); the environment is
            stepped with it, the reward discarded; on to the child.
  Terminal  s has edges and len(s) + 1 == D: a' is drawn, value = Qsa[(s, a')]; the counted edge is (s, 0), not (s, a'), and its Q is
            NOT updated (the reference's best_act quirk).
  Counting  at the node where the walk ended and at every node on the way back up: Ns += 1, Nsa[edge] += 1 and, unless it is the
            terminal edge, Q = (Q (n - 1) + value) / n.
The result is the first-index argmax of the root's Nsa.  Rewards are minus collision counts, so every Q is built from integers.

Draws.  A batch cannot reproduce the order in which the recursion consumes the global stream, so the batched search reads a table
draws (T, runs, D) int32 in [0, A): iteration i of tree t reads row (t, i) from column 0 on -- Expand column 0 for its action and
columns 1 .. D - len(s) for the rollout, Terminal column 0 only.
Replicas.  R independent trees per environment: T = M R, tree m R + k starts from environment m's state with its own rows of the
table, and the action of environment m is the first-index argmax of the root counts summed over its R trees.  R = 1 is the reference.
Lock step.  Every iteration replays its path from the root state, as the reference does (env_reset), so an Expand iteration is
exactly D environment steps at any depth and a Terminal one D - 2: all trees are at step k of iteration i together, and a tree needs
only the root state and the tree arrays -- no per-node state pool.

Array layout (Forest's): slot 0 the root; expanding a node takes A consecutive slots; slot first[s] + a holds the edge (s, a) -- Qsa,
Nsa -- and the node s + str(a) -- Ns, first, parent, depth (= len - 1).  cap = 1 + A runs always suffices.  Per tree: status (0
searched; 1 out of slots, frozen; 2 a draw outside [0, A) or a failed index check, the tree left as it stood at the start of that
iteration and frozen) and gap, the smallest u_best - u_a over all Descend levels among a whose (Qsa, Nsa) differ from the best's
(equal inputs tie exactly on every side and do not count): log is a library call, so two sides take the same decisions when it is
well above a rounding error."""
import numpy as np
import torch

from ..envs.batched import ACTIONS, BatchedAvoidance
from .mcts_stove import Forest


class MCTS:
    """the reference's per-environment search: MCTS(env).run_mcts(runs) -> the most visited root action.  Nsa, Qsa: {(s, a): .};
    Ns: {s: .}.  The environment is stepped in place and put back to the root state after every iteration."""

    def __init__(self, env, max_rollout=20):
        if max_rollout < 2:
            raise ValueError('the search needs max_rollout >= 2, not %r (the reference fails with a KeyError there)' % (max_rollout,))
        self.env = env
        self.root_x = np.array(env.env.x, copy=True)
        self.root_v = np.array(env.env.v, copy=True)
        self.actions = env.get_action_space()
        self.Nsa, self.Qsa, self.Ns = {}, {}, {'r': 0}
        self.c = 1.
        self.max_rollout = max_rollout

    def run_mcts(self, runs_per_round):
        for _ in range(runs_per_round):
            self.select(self.env, 'r')
            self.env_reset()
        return int(np.argmax([self.Nsa.get(('r', a), 0) for a in range(self.actions)]))

    def select(self, env, s):
        """one level of the walk at node s -> the value handed back up"""
        edge, counted_q = 0, True
        if (s, 0) not in self.Qsa and len(s) != self.max_rollout:
            edge, value = self.expand(s, env)
        elif len(s) + 1 != self.max_rollout:
            best = -float('inf')
            for a in range(self.actions):
                u = self.Qsa[(s, a)] + self.c * np.sqrt(np.log(self.Ns[s]) / (1 + self.Nsa[(s, a)]))
                if u > best:
                    best, edge = u, a
            env.step(edge)
            value = self.select(env, s + str(edge))
        else:
            value = self.Qsa[(s, np.random.randint(self.actions))]
            counted_q = False
        self.Ns[s] += 1
        self.Nsa[(s, edge)] += 1
        if counted_q:
            n = self.Nsa[(s, edge)]
            self.Qsa[(s, edge)] = (self.Qsa[(s, edge)] * (n - 1) + value) / n
        return value

    def expand(self, s, env):
        """-> (the drawn action, its reward plus the rollout's)"""
        self.Ns[s] = 0
        for a in range(self.actions):
            self.Qsa[(s, a)] = -1
            self.Nsa[(s, a)] = 0
        a = np.random.randint(self.actions)
        r = env.step(a)[2]
        return a, r + self.rollout(env, len(s))

    def rollout(self, env, cur_depth):
        total = 0
        for _ in range(self.max_rollout - cur_depth):
            total += env.step(np.random.randint(self.actions))[2]
        return total

    def env_reset(self):
        self.env.env.x = np.array(self.root_x, copy=True)
        self.env.env.v = np.array(self.root_v, copy=True)


_WALK, _ROLL, _TERM, _FULL, _BAD, _FROZEN = range(6)


class EnvForest(Forest):
    """T trees searched in lock step on the rows of a host BatchedAvoidance (its _step_rows): the yardstick of the device search."""

    def __init__(self, T, actions=ACTIONS, max_rollout=10, runs=100):
        if max_rollout < 2:
            raise ValueError('the search needs max_rollout >= 2, not %r' % (max_rollout,))
        if actions != ACTIONS:
            raise ValueError('the avoidance environments have %d actions, not %r' % (ACTIONS, actions))
        super().__init__(T, actions, max_rollout, cap=1 + actions * runs)
        self.runs = runs
        self.status = np.zeros(T, dtype=np.int32)
        self.gap = np.full(T, np.inf)

    def to_device(self, dev):
        """-> dict of device tensors for ops.env_search (Forest.to_device, with this forest's status and per-tree gaps)"""
        out = super().to_device(dev)
        out['status'] = torch.from_numpy(self.status.astype(np.int32)).to(dev)
        out['min_gap'] = torch.from_numpy(self.gap.copy()).to(dev)
        return out

    def from_device(self, tensors):
        super().from_device(tensors)
        self.status = tensors['status'].cpu().numpy().astype(np.int32)
        self.gap = tensors['min_gap'].cpu().numpy().astype(np.float64)

    # -------------------------------------------------------------------------------------------- the search
    def search(self, envs, draws, replicas=1):
        """all draws.shape[1] iterations of every tree from the states of `envs` (a host BatchedAvoidance of T / replicas environments,
        left untouched) -> action (M,) int32"""
        if envs.device is not None:
            raise ValueError('EnvForest searches a host BatchedAvoidance (the device search is ops.env_search)')
        R = int(replicas)
        draws = np.asarray(draws)
        if R < 1 or envs.M * R != self.M or draws.ndim != 3 or draws.shape[0] != self.M or draws.shape[2] != self.D:
            raise ValueError('EnvForest.search: %d trees of depth %d need replicas x %d environments and draws (T, runs, D), not %s'
                             % (self.M, self.D, envs.M, draws.shape))
        env_of = np.arange(self.M) // R
        root = tuple(getattr(envs, k)[env_of] for k in ('x', 'v', 'r', 'm'))
        for i in range(draws.shape[1]):
            self._iterate(envs, root, draws[:, i].astype(np.int64))
        return self.actions_of(R)

    def _iterate(self, envs, root, draws):
        """env_search.h: iterate, for every tree at once; a branch of the header is a mask here"""
        T, A, D, cap = self.M, self.A, self.D, self.cap
        rows, steps = np.arange(T), np.arange(A)
        x, v = root[0].copy(), root[1].copy()
        r, m = root[2], root[3]
        mode = np.where(self.status == 0, _WALK, _FROZEN)
        cur, col, fresh, edge_a, hits = (np.zeros(T, dtype=np.int64) for _ in range(5))
        value, gap = np.zeros(T), np.full(T, np.inf)
        for k in range(D):
            act = np.zeros(T, dtype=np.int64)
            going = np.zeros(T, dtype=bool)
            roll = rows[mode == _ROLL]
            act[roll] = draws[roll, col[roll]]
            col[roll] += 1
            going[roll] = True
            w = rows[mode == _WALK]
            down = w[:0]
            if w.size:
                c = cur[w]
                fc, used = self.first[w, c], self.used[w]
                wrong = self.depth[w, c] != k
                fresh_leaf = ~wrong & (fc < 0)
                wrong |= fresh_leaf & ((k + 1 >= D) | (used < 1) | (used > cap))
                full = fresh_leaf & ~wrong & (used > cap - A)
                inner = ~wrong & (fc >= 0)
                wrong |= inner & ((fc < 1) | (fc > cap - A))
                e = w[fresh_leaf & ~wrong & ~full]                         # Expand
                fresh[e] = self.used[e]
                act[e] = edge_a[e] = draws[e, 0]
                col[e] = 1
                mode[e] = _ROLL
                going[e] = True
                inner &= ~wrong
                if k + 2 != D:                                             # Descend
                    g, cg, fg = w[inner], c[inner], fc[inner]
                    ch, tree = fg[:, None] + steps, g[:, None]
                    q, n = self.Qsa[tree, ch], self.Nsa[tree, ch]
                    with np.errstate(divide='ignore', invalid='ignore'):
                        u = q + self.c * np.sqrt(np.log(self.Ns[g, cg])[:, None] / (1 + n))
                    best_u, best = np.full(g.size, -np.inf), np.zeros(g.size, dtype=np.int64)
                    for a in range(A):
                        better = u[:, a] > best_u
                        best_u, best = np.where(better, u[:, a], best_u), np.where(better, a, best)
                    i = np.arange(g.size)
                    same = (q == q[i, best][:, None]) & (n == n[i, best][:, None])
                    with np.errstate(invalid='ignore'):
                        gap[g] = np.minimum(gap[g], np.where(same, np.inf, best_u[:, None] - u).min(1, initial=np.inf))
                    lost = self.parent[g, fg + best] != cg
                    mode[g[lost]] = _BAD
                    down = g[~lost]
                    act[down] = best[~lost]
                    going[down] = True
                else:                                                      # Terminal
                    g, fg = w[inner], fc[inner]
                    a = draws[g, 0]
                    fine = (a >= 0) & (a < A)
                    value[g[fine]] = self.Qsa[g[fine], fg[fine] + a[fine]]
                    mode[g[fine]] = _TERM
                    mode[g[~fine]] = _BAD
                mode[w[wrong]] = _BAD
                mode[w[full]] = _FULL
            refused = going & ((act < 0) | (act >= A))
            mode[refused] = _BAD
            going &= ~refused
            s = rows[going]
            if s.size:
                xs, vs = x[s], v[s]
                hit = envs._step_rows(xs, vs, r[s], m[s], act[s])
                x[s], v[s] = xs, vs
                counted = mode[s] == _ROLL
                hits[s[counted]] += hit[counted]
            down = down[going[down]]
            cur[down] = self.first[down, cur[down]] + act[down]
        mode[mode == _WALK] = _BAD
        self.status[mode == _FULL] = 1
        self.status[mode == _BAD] = 2
        # ---- the iterations that count: expansion, then counts and means from the node where the walk ended up to the root
        e = rows[mode == _ROLL]
        ch, tree = fresh[e][:, None] + steps, e[:, None]
        self.first[tree, ch] = -1
        self.parent[tree, ch] = cur[e][:, None]
        self.depth[tree, ch] = self.depth[e, cur[e]][:, None] + 1
        self.Qsa[tree, ch] = -1.0
        self.Nsa[tree, ch] = 0
        self.Ns[tree, ch] = 0
        self.first[e, cur[e]] = fresh[e]
        self.Ns[e, cur[e]] = 0
        self.used[e] = fresh[e] + A
        value[e] = (-hits[e]).astype(np.float64)
        edge = np.zeros(T, dtype=np.int64)
        edge[e] = fresh[e] + edge_a[e]
        t = rows[mode == _TERM]
        edge[t] = self.first[t, cur[t]]
        ok = rows[(mode == _ROLL) | (mode == _TERM)]
        self.Ns[ok, cur[ok]] += 1
        self.Nsa[ok, edge[ok]] += 1
        n = self.Nsa[e, edge[e]]
        self.Qsa[e, edge[e]] = (self.Qsa[e, edge[e]] * (n - 1) + value[e]) / n
        node = cur.copy()
        up = np.zeros(T, dtype=bool)
        while True:
            up[:] = False
            up[ok] = self.depth[ok, node[ok]] >= 1
            if not up.any():
                break
            g, nd = rows[up], node[up]
            par = self.parent[g, nd]
            self.Ns[g, par] += 1
            self.Nsa[g, nd] += 1
            self.Qsa[g, nd] = (self.Qsa[g, nd] * (self.Nsa[g, nd] - 1) + value[up]) / self.Nsa[g, nd]
            node[up] = par
        self.gap[ok] = np.minimum(self.gap[ok], gap[ok])
        if ok.size:
            self.min_gap = min(self.min_gap, float(self.gap[ok].min()))

    def actions_of(self, replicas=1):
        """-> (T / replicas,) int32: the first-index argmax of the root's visit counts summed over each environment's trees"""
        fc = self.first[:, 0]
        has = (fc >= 1) & (fc <= self.cap - self.A)
        counts = np.zeros((self.M, self.A), dtype=np.int64)
        g = np.flatnonzero(has)
        counts[g] = self.Nsa[g[:, None], fc[g][:, None] + np.arange(self.A)]
        return counts.reshape(self.M // replicas, replicas, self.A).sum(1).argmax(1).astype(np.int32)


def plan_on_envs(envs, mcts_steps=100, max_rollout_depth=10, replicas=1, draws=None):
    """One planning step on a BatchedAvoidance, searched where it lives: EnvForest on the host, one ops.env_search on a device.
    draws (M replicas, mcts_steps, max_rollout_depth) in [0, 9), or None: one np.random.randint(9, size=...) from the global stream.
    The environments are left untouched.  -> list of M action indices; RuntimeError if any tree's status is non-zero."""
    if not isinstance(envs, BatchedAvoidance):
        raise ValueError('plan_on_envs searches a BatchedAvoidance (BatchedAvoidance.from_tasks makes one of a list of AvoidanceTask)')
    D, R, runs = int(max_rollout_depth), int(replicas), int(mcts_steps)
    if D < 2:
        raise ValueError('the search needs max_rollout_depth >= 2, not %r' % (max_rollout_depth,))
    if R < 1 or runs < 0:
        raise ValueError('the search needs replicas >= 1 and mcts_steps >= 0')
    T = envs.M * R
    if draws is None:
        draws = np.random.randint(ACTIONS, size=(T, runs, D))
    draws = np.asarray(draws)
    if draws.shape != (T, runs, D):
        raise ValueError('draws is %s, the search needs %s' % (draws.shape, (T, runs, D)))
    forest = EnvForest(T, ACTIONS, D, runs)
    if envs.device is None:
        action = forest.search(envs, draws, R)
        status = forest.status
    else:
        from .. import ops
        arrays = forest.to_device(envs.device)
        table = torch.from_numpy(np.ascontiguousarray(draws, dtype=np.int32)).to(envs.device)
        action = ops.env_search(envs.x, envs.v, envs.r, envs.m, table, arrays, D, envs.granularity, envs.hw, envs.t, envs.friction,
                                envs.action_force, envs.drift, replicas=R).cpu().numpy()
        status = arrays['status'].cpu().numpy()
    if status.any():
        bad = int(np.flatnonzero(status)[0])
        raise RuntimeError('tree %d of the search ended with status %d' % (bad, int(status[bad])))
    return [int(a) for a in action]
