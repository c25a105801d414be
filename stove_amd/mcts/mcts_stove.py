"""Monte-Carlo tree search on the learned world model (reference model/mcts/mcts_stove.py), batched over the trees.

The reference keeps every tree as dictionaries keyed by action strings ('r', 'r3', 'r31', ...) and walks them one tree at a time in a
process pool.  Here the trees of a batch live in one `Forest`: numpy arrays (M, cap) of first-child slot, Ns, Nsa, Qsa, parent and
depth, walked one tree LEVEL at a time for all trees at once, in float64 -- the reference's `select` and `backpropagate` are the
specification, quirks included (`cur_best` / `best_act` carried from level to level, strict `>`, c = 1, the broadcast product in the
value).  The node states live in a pool tensor (M, cap, N, 18): slot 0 is the root, an expansion appends A consecutive child slots.
`MCTS` stays the per-tree handle: `tree.Nsa['r3']`, `tree.Qsa`, `tree.Ns`, `tree.Zstate` read the forest by the reference's keys.

`BatchedMCTSHandler.run_mcts` expands with one `ops.plan_expand` call per iteration (fused=True: the states never leave the device)
or with the reference's sequence of calls on `Stove.rollout` (fused=False).  With `handler.device_trees = True` the forest itself goes to the device
for the length of the search (`Forest.to_device`, one `ops.plan_search` call for all iterations, `Forest.from_device`)."""
import time

import numpy as np
import torch

GAMMA = 0.95
# What run_mcts(fused=None) takes on a model the fused expansion serves (cl = 32, float32, on the GPU, fused reward head).  The fused
# path may be the default only where tools/plan_bench.py has shown it faster than the composed one beyond the run-to-run spread.
# profiles/plan_bench.json records 1.10 against 3.68 ms per expansion; the default is the composed path all the same.
FUSED_WHERE_ELIGIBLE = False
# The state-code lengths the fused expansion and the device-resident search are offered at.  The kernels serve 16, 32 and 64
# (ops.plan_expand / ops.plan_search); 16 and 64 are switched on per handler (handler.fused_widths, the `fused_widths` keyword of
# plan_on_model / plan_on_frames / play, tools/run_mcts.py --fused-widths), so that a model of those widths keeps taking the composed
# path, and keeps being refused by device_trees = True, unless it is asked for.
FUSED_WIDTHS = (32,)
# what the kernels of a width take: (object count, appearance columns) -- csrc/validate.h: plan_dims_bad; the table is held to the
# library's workspace queries by tests/test_plan_cl_cpu.py
_FUSED_LIMITS = {16: (6, 4), 32: (8, 12), 64: (6, 28)}


def multi_one_hot(actions, action_shape):
    """list of action indices -> (1, len, action_shape) one-hot rows"""
    n = len(actions)
    full_vec = torch.zeros((n, action_shape))
    full_vec[range(n), actions] = 1.
    return full_vec.unsqueeze(0)


def tile(a, dim, n_tile):
    """repeat_interleave along `dim` (the reference's helper of that name)"""
    return torch.repeat_interleave(a, n_tile, dim=dim)


def encode_img(img):
    """(batch, time, width, height, channels) numpy frames -> (batch, time, channels, width, height) tensor"""
    return torch.Tensor(img).permute(0, 1, 4, 2, 3)


def discounted_values(rs, r_rollout, len_s, max_rollout, gamma=GAMMA):
    """The reference's value of every new child (mcts_stove.py:186-196) in float64: rs (..., A) rewards of the expanding step,
    r_rollout (..., A, L) of the random rollout, len_s (...) key lengths ->
        (rs - 1) gamma^len_s + sum_{k < 2 D - len_s + 1} (r_k - 1) * sum_{j = len_s}^{D - 1} gamma^j
    -- the reference multiplies (remaining, 1) rewards with (D - len_s,) discounts, which broadcasts to the product of the two sums."""
    rs = np.asarray(rs, dtype=np.float64) - 1.0
    rr = np.asarray(r_rollout, dtype=np.float64) - 1.0
    len_s = np.asarray(len_s, dtype=np.int64)
    remaining = max_rollout * 2 - len_s + 1
    assert (remaining >= 0).all()
    counted = np.arange(rr.shape[-1]) < remaining[..., None, None]
    s1 = np.where(counted, rr, 0.0).sum(-1)
    j = np.arange(max_rollout)
    s2 = np.where(j >= len_s[..., None], gamma ** j.astype(np.float64), 0.0).sum(-1)
    return rs * (gamma ** len_s.astype(np.float64))[..., None] + s1 * s2[..., None]


class Forest:
    """M search trees as arrays (M, cap): slot 0 of a tree is its root 'r'; expanding a node appends A consecutive slots."""

    def __init__(self, num_trees, actions, max_rollout, cap=0, c=1.0):
        self.M, self.A, self.D, self.c = num_trees, actions, max_rollout, c
        cap = max(cap, 1 + actions)
        self.first = np.full((num_trees, cap), -1, dtype=np.int64)
        self.parent = np.full((num_trees, cap), -1, dtype=np.int64)
        self.depth = np.zeros((num_trees, cap), dtype=np.int64)            # the reference's len(key) - 1
        self.Ns = np.zeros((num_trees, cap), dtype=np.int64)
        self.Nsa = np.zeros((num_trees, cap), dtype=np.int64)
        self.Qsa = np.zeros((num_trees, cap), dtype=np.float64)
        self.used = np.ones(num_trees, dtype=np.int64)
        self.z = None                  # (M, cap, N, 18) node states, wherever the search runs
        self.min_gap = float('inf')    # smallest best-minus-second-best UCT value over all decisions taken so far

    _ARRAYS = ('first', 'parent', 'depth', 'Ns', 'Nsa', 'Qsa')
    _FILL = {'first': -1, 'parent': -1}

    @property
    def cap(self):
        return self.first.shape[1]

    def reserve(self, cap):
        """room for `cap` slots per tree (arrays and state pool)"""
        if cap > self.cap:
            for name in self._ARRAYS:
                old = getattr(self, name)
                new = np.full((self.M, cap), self._FILL.get(name, 0), dtype=old.dtype)
                new[:, :old.shape[1]] = old
                setattr(self, name, new)
        if self.z is not None and self.z.shape[1] < cap:
            z = torch.zeros((self.M, cap) + tuple(self.z.shape[2:]), dtype=self.z.dtype, device=self.z.device)
            z[:, :self.z.shape[1]] = self.z
            self.z = z

    @classmethod
    def merged(cls, forests):
        """one forest holding the trees of `forests`, in order"""
        f0 = forests[0]
        out = cls(sum(f.M for f in forests), f0.A, f0.D, max(f.cap for f in forests), f0.c)
        row = 0
        for f in forests:
            if (f.A, f.D) != (f0.A, f0.D):
                raise ValueError('trees of one batch need the same action space and rollout depth')
            for name in cls._ARRAYS:
                getattr(out, name)[row:row + f.M, :f.cap] = getattr(f, name)
            out.used[row:row + f.M] = f.used
            out.min_gap = min(out.min_gap, f.min_gap)
            row += f.M
        zs = [f.z for f in forests]
        if all(z is not None for z in zs):
            dev = zs[0].device
            out.z = torch.zeros((out.M, out.cap) + tuple(zs[0].shape[2:]), dtype=zs[0].dtype, device=dev)
            row = 0
            for f in forests:
                out.z[row:row + f.M, :f.z.shape[1]] = f.z.to(dev)
                row += f.M
        return out

    # -------------------------------------------------------------------------------------------- the trees on the device
    def to_device(self, dev):
        """-> dict of device tensors for ops.plan_search: the arrays as int32 (Qsa float64), used and a zero status (M,) int32, and
        min_gap (M,) float64 at +inf (the search lowers it per tree)"""
        out = {}
        for name in self._ARRAYS + ('used',):
            a = getattr(self, name)
            if name != 'Qsa':
                if a.size and (a.max() > np.iinfo(np.int32).max or a.min() < np.iinfo(np.int32).min):
                    raise ValueError('Forest.to_device: %s does not fit int32' % name)
                a = a.astype(np.int32)
            out[name] = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        out['status'] = torch.zeros(self.M, dtype=torch.int32, device=dev)
        out['min_gap'] = torch.full((self.M,), float('inf'), dtype=torch.float64, device=dev)
        return out

    def from_device(self, tensors):
        """the arrays of `to_device` after a search, back into this forest (int64 / float64 numpy); min_gap merged with min"""
        for name in self._ARRAYS + ('used',):
            a = tensors[name].cpu().numpy()
            want = (self.M, self.cap) if name != 'used' else (self.M,)
            if a.shape != want:
                raise ValueError('Forest.from_device: %s is %s, this forest holds %s' % (name, a.shape, want))
            setattr(self, name, a.astype(np.float64 if name == 'Qsa' else np.int64))
        gaps = tensors['min_gap'].cpu().numpy()
        if gaps.size:
            self.min_gap = min(self.min_gap, float(gaps.min()))

    # -------------------------------------------------------------------------------------------- the reference's select
    def select(self, start=None):
        """-> leaf slot (M,) of every tree.  One pass per tree level: the UCT values of the A children of every tree still
        descending, then the reference's scan `if u > cur_best` over the actions with cur_best / best_act carried along."""
        M, A = self.M, self.A
        rows = np.arange(M)
        cur = np.zeros(M, dtype=np.int64) if start is None else np.asarray(start, dtype=np.int64).copy()
        cur_best = np.full(M, -np.inf)
        best_act = np.zeros(M, dtype=np.int64)
        steps = np.arange(A)
        while True:
            fc = self.first[rows, cur]
            go = (fc >= 0) & (self.depth[rows, cur] + 1 != self.D)
            if not go.any():
                return cur
            g = rows[go]
            ch = fc[go][:, None] + steps
            tree = g[:, None]
            with np.errstate(divide='ignore', invalid='ignore'):
                u = self.Qsa[tree, ch] + self.c * np.sqrt(np.log(self.Ns[g, cur[go]])[:, None] / (1 + self.Nsa[tree, ch]))
            cb, ba = cur_best[go], best_act[go]
            cand = np.sort(np.concatenate([cb[:, None], u], 1), 1)
            gaps = cand[:, -1] - cand[:, -2]
            gaps = gaps[np.isfinite(gaps)]
            if gaps.size:
                self.min_gap = min(self.min_gap, float(gaps.min()))
            for a in range(A):
                better = u[:, a] > cb
                cb = np.where(better, u[:, a], cb)
                ba = np.where(better, a, ba)
            cur_best[go], best_act[go] = cb, ba
            cur[go] = fc[go] + ba

    def child_slots(self, leaf):
        """-> first child slot (M,) of every tree's `leaf`: the slots it already has (a leaf at the depth limit is expanded again
        and again, and the reference overwrites its children) or A fresh ones"""
        rows = np.arange(self.M)
        have = self.first[rows, leaf]
        child = np.where(have >= 0, have, self.used)
        fresh = have < 0
        need = int((self.used + np.where(fresh, self.A, 0)).max())
        if need > self.cap:
            self.reserve(max(need, 2 * self.cap))
        self.used = self.used + np.where(fresh, self.A, 0)
        return child

    # -------------------------------------------------------------------------------------------- the reference's backpropagate
    def backpropagate(self, leaf, child, q):
        """q (M, A) float64: the new children's values.  Children (re)initialised, then the mean value walks up to the root's child."""
        M, A = self.M, self.A
        rows = np.arange(M)
        ch = child[:, None] + np.arange(A)
        tree = rows[:, None]
        self.first[rows, leaf] = child
        self.parent[tree, ch] = leaf[:, None]
        self.depth[tree, ch] = self.depth[rows, leaf][:, None] + 1
        self.first[tree, ch] = -1
        self.Qsa[tree, ch] = q
        self.Nsa[tree, ch] = 1
        self.Ns[tree, ch] = 0
        self.Ns[rows, leaf] += 1
        total = np.zeros(M)
        for a in range(A):                     # the reference's running sum, in its order
            total = total + q[:, a]
        value = total / A
        node = leaf.copy()
        while True:
            up = self.depth[rows, node] >= 1
            if not up.any():
                return
            g, n = rows[up], node[up]
            par = self.parent[g, n]
            self.Ns[g, par] += 1
            self.Nsa[g, n] += 1
            self.Qsa[g, n] = (self.Qsa[g, n] * (self.Nsa[g, n] - 1) + value[up]) / self.Nsa[g, n]
            node[up] = par

    # -------------------------------------------------------------------------------------------- the reference's keys
    def slot_of(self, m, key):
        """slot of the reference's key ('r' + one digit per action), or -1"""
        if not key or key[0] != 'r':
            return -1
        slot = 0
        for ch in key[1:]:
            fc = self.first[m, slot]
            if fc < 0 or not ch.isdigit() or int(ch) >= self.A:
                return -1
            slot = fc + int(ch)
        return int(slot)

    def key_of(self, m, slot):
        digits = []
        while self.depth[m, slot] >= 1:
            par = self.parent[m, slot]
            digits.append(str(int(slot - self.first[m, par])))
            slot = par
        return 'r' + ''.join(reversed(digits))

    def keys(self, m):
        """every key of tree m, parents before children"""
        out, stack = [], [(0, 'r')]
        while stack:
            slot, key = stack.pop()
            out.append(key)
            fc = self.first[m, slot]
            if fc >= 0:
                stack.extend((fc + a, key + str(a)) for a in reversed(range(self.A)))
        return out


class _KeyView:
    """tree.Nsa / tree.Qsa / tree.Ns / tree.Zstate by the reference's string keys, read from the forest"""

    def __init__(self, tree, name):
        self._t, self._name = tree, name

    def _slot(self, key):
        slot = self._t._f.slot_of(self._t._m, key)
        if slot < 0:
            raise KeyError(key)
        return slot

    def __getitem__(self, key):
        f, m, slot = self._t._f, self._t._m, self._slot(key)
        if self._name == 'Zstate':
            return f.z[m, slot].unsqueeze(0).cpu()
        return getattr(f, self._name)[m, slot].item()

    def __contains__(self, key):
        return self._t._f.slot_of(self._t._m, key) >= 0

    def keys(self):
        return self._t._f.keys(self._t._m)

    def __iter__(self):
        return iter(self.keys())


class MCTS():
    """One search tree: the reference's constructor, `select` and `backpropagate`; the numbers live in a Forest (its own of one tree
    until a BatchedMCTSHandler merges the trees of a batch into one)."""

    def __init__(self, appearance, inferred_z, action_space=9, max_rollout_depth=20):
        self.actions = action_space
        self.c = 1.
        self.gamma = GAMMA
        self.app = appearance.cpu() if appearance is not None else None
        self.max_rollout = max_rollout_depth
        self._f = Forest(1, action_space, max_rollout_depth, c=self.c)
        self._m = 0
        z = torch.as_tensor(inferred_z).detach().cpu()
        z = z.reshape(z.shape[-2:])
        self._f.z = torch.zeros((1, self._f.cap) + tuple(z.shape), dtype=z.dtype)
        self._f.z[0, 0] = z
        self.Nsa, self.Qsa, self.Ns, self.Zstate = (_KeyView(self, n) for n in ('Nsa', 'Qsa', 'Ns', 'Zstate'))

    def _own(self):
        if self._f.M != 1:
            raise RuntimeError('this tree belongs to a batch: search it through its BatchedMCTSHandler')
        return self._f

    def select(self, s='r', z=None):
        """-> (key of the selected leaf, its state (1, N, 18))"""
        f = self._own()
        start = f.slot_of(0, s)
        if start < 0:
            raise KeyError(s)
        leaf = int(f.select(np.array([start]))[0])
        return f.key_of(0, leaf), f.z[0, leaf].unsqueeze(0).cpu()

    def backpropagate(self, new_zs, rs, r_rollout, s):
        """new_zs (A, 1, N, 18) child states, rs (A, 1, 1) their rewards, r_rollout (A, 2 D, 1) the random rollouts' rewards, s the
        expanded key"""
        f = self._own()
        leaf = f.slot_of(0, s)
        if leaf < 0:
            raise KeyError(s)
        rs = np.asarray(torch.as_tensor(rs).detach().cpu().numpy()).reshape(self.actions)
        rr = np.asarray(torch.as_tensor(r_rollout).detach().cpu().numpy()).reshape(self.actions, -1)
        q = discounted_values(rs[None], rr[None], np.array([len(s)]), self.max_rollout, self.gamma)
        leaf = np.array([leaf])
        child = f.child_slots(leaf)
        f.backpropagate(leaf, child, q)
        zs = torch.as_tensor(new_zs).detach().reshape((self.actions,) + tuple(f.z.shape[2:]))
        f.z[0, int(child[0]):int(child[0]) + self.actions] = zs.to(f.z)


class BatchedMCTSHandler():
    """Holds a batch of MCTS trees and runs them concurrently on the model."""

    def __init__(self, trees, appearances, action_space=9, max_rollout_depth=20):
        self.num_mcts = len(trees)
        self.trees = trees
        self.max_rollout = max_rollout_depth
        self.obj_app = appearances
        self.actions = action_space
        self.forest = Forest.merged([t._f for t in trees])
        for m, t in enumerate(trees):
            t._f, t._m = self.forest, m
        self.timing = {'host': 0.0, 'device': 0.0}        # seconds of the last run_mcts: tree arithmetic / waiting for the model
        self.device_trees = False      # True: run_mcts keeps the trees on the device too, one ops.plan_search call per search
        self.fused_widths = FUSED_WIDTHS        # the state-code lengths _fused_unserved lets onto the fused expansion

    def _fused_default(self, env):
        c = env.c
        p = next(env.parameters())
        return bool(FUSED_WHERE_ELIGIBLE and p.is_cuda and p.dtype == torch.float32 and c.cl == 32 and c.action_conditioned and getattr(c, 'fused_reward_head', True))

    def run_mcts(self, env, runs_per_round, fused=None, rollout_actions=None):
        """Expand every tree `runs_per_round` times on the model `env` (an action-conditioned Stove) -> the next action of every tree,
        the argmax of its root's visit counts.
        fused: True -- one ops.plan_expand per iteration, node states resident on the device, per iteration only leaf / child / len_s
        go up and q (M, A) comes down; False -- the reference's sequence of calls on Stove.rollout; None -- fused where the model is
        cl = 32, float32, on the GPU with its fused reward head and the fused path was measured faster (FUSED_WHERE_ELIGIBLE), else composed.
        rollout_actions: (runs_per_round, M A, 2 D) action indices of the random rollouts; None draws them as the reference does, one
        np.random.randint(A, size=(A M 2 D,)) per iteration (drawn ahead of the loop, in that order: the loop draws nothing else).
        self.device_trees (an attribute of the handler, False by default; this method's parameters are the reference's plus `fused`
        and `rollout_actions` and stay so): True -- the trees go to the device too and all iterations are ONE ops.plan_search call (select and backpropagate
        as kernels around the fused expansion's launches, nothing synchronised in between); the forest is uploaded before and
        downloaded after, so it reads as if searched on the host.  Implies the fused expansion; a model that one does not serve is a
        ValueError.
        self.fused_widths (an attribute too, FUSED_WIDTHS = (32,) by default): the state-code lengths the fused expansion is offered
        at.  A cl = 16 / 64 model takes fused=True or device_trees = True only with its width in there (else the ValueError above)."""
        device_trees = bool(self.device_trees)
        if device_trees:
            if fused is False:
                raise ValueError('device_trees = True searches on the fused expansion: fused=False contradicts it')
            why = self._fused_unserved(env, self.fused_widths)
            if why:
                raise ValueError('device_trees=True needs the fused expansion, which does not serve this model: ' + why)
            fused = True
        if fused is None:
            fused = self._fused_default(env)
        elif fused and (env.c.cl != 32 or 32 not in self.fused_widths):
            # a width is served where the handler offers it, under fused=True as under device_trees.  (A cl = 16 / 64 model asked for
            # with fused=True used to get as far as ops.plan_expand and its 'do not fit'; it is now refused here, by name.)
            why = self._fused_unserved(env, self.fused_widths)
            if why:
                raise ValueError('fused=True asks for the fused expansion, which does not serve this model: ' + why)
        if not env.c.action_conditioned:
            raise ValueError('planning needs an action-conditioned model (rewards)')
        M, A, D, f = self.num_mcts, self.actions, self.max_rollout, self.forest
        L = 2 * D
        if rollout_actions is None:
            rollout_actions = np.stack([np.random.randint(A, size=(A * M * D * 2,)) for _ in range(runs_per_round)]) if runs_per_round else \
                np.zeros((0, M * A * L), dtype=np.int64)
        acts_all = np.asarray(rollout_actions).reshape(runs_per_round, M * A, L)
        dev = next(env.parameters()).device
        f.reserve(int(f.used.max()) + A * runs_per_round)
        f.z = f.z.to(dev).float().contiguous()
        app = self.obj_app.to(dev).float().contiguous() if self.obj_app is not None else None
        if device_trees:
            return self._search_on_device(env, acts_all, app)
        expand = self._expand_fused(env, acts_all, app) if fused else self._expand_composed(env, acts_all, app)
        host = device = 0.0
        with torch.no_grad():
            for i in range(runs_per_round):
                t0 = time.perf_counter()
                leaf = f.select()
                child = f.child_slots(leaf)
                len_s = f.depth[np.arange(M), leaf] + 1
                t1 = time.perf_counter()
                q = expand(i, leaf, child, len_s)
                t2 = time.perf_counter()
                f.backpropagate(leaf, child, q)
                host += t1 - t0 + time.perf_counter() - t2
                device += t2 - t1
        self.timing = {'host': host, 'device': device}
        return [int(np.argmax(f.Nsa[m, f.first[m, 0]:f.first[m, 0] + A])) if f.first[m, 0] >= 0 else 0 for m in range(M)]

    @staticmethod
    def _fused_unserved(env, widths=None):
        """why the fused expansion (stove_plan_expand[_cl]) does not serve `env`, or '' if it does.  widths: the state-code lengths
        offered (a handler passes its fused_widths; None: FUSED_WIDTHS)"""
        c = env.c
        p = next(env.parameters())
        if not p.is_cuda:
            return 'it is not on the GPU'
        if p.dtype != torch.float32:
            return 'its parameters are %s, not float32' % p.dtype
        widths = FUSED_WIDTHS if widths is None else tuple(widths)
        if c.cl not in widths or c.cl not in _FUSED_LIMITS:
            return 'its state code length is %d, not %s' % (c.cl, ' or '.join(str(w) for w in sorted(set(widths) & set(_FUSED_LIMITS))))
        max_obj, max_app = _FUSED_LIMITS[c.cl]
        app_dim = c.debug_appearance_dim if getattr(c, 'debug_core_appearance', False) else 0
        if c.num_obj > max_obj:
            return 'it has %d objects, the kernels of state code length %d take at most %d' % (c.num_obj, c.cl, max_obj)
        if app_dim > max_app:
            return 'its core reads %d appearance columns, the kernels of state code length %d take at most %d' % (app_dim, c.cl, max_app)
        return ''

    @staticmethod
    def _fused_weights(env):
        """what stove_plan_expand[_cl] reads of the model: embedding, GNN image of its state-code length, reward-head block"""
        from .. import ops
        dyn = env.dyn
        lay, h0, h1 = dyn.action_embedding_layer, dyn.reward_head0, dyn.reward_head1
        gnn = ops.gnn_width(env.c.cl).image(*[t.detach() if t is not None else None for t in dyn.kernel_params(0)[0]]).contiguous()
        rh = torch.cat([p.detach().float().reshape(-1) for p in (h0[0].weight, h0[0].bias, h0[2].weight, h0[2].bias, h1[0].weight, h1[0].bias,
                                                                  h1[2].weight, h1[2].bias, h1[4].weight, h1[4].bias)])
        return lay.weight.detach().float().contiguous(), lay.bias.detach().float().contiguous(), gnn, rh

    def _search_on_device(self, env, acts_all, app):
        """all iterations in one ops.plan_search call: forest up, search, forest down -> the actions"""
        from .. import ops
        dyn, f = env.dyn, self.forest
        dev = f.z.device
        if f.c != 1.0:
            raise ValueError('the device search runs the reference\'s exploration constant c = 1, this forest has c = %r' % f.c)
        t0 = time.perf_counter()
        with torch.no_grad():
            emb_w, emb_b, gnn, rh = self._fused_weights(env)
            acts = torch.from_numpy(acts_all.astype(np.int32)).to(dev)
            arrays = f.to_device(dev)
            action = ops.plan_search(f.z, arrays, app, acts, emb_w, emb_b, gnn, rh, self.max_rollout, 2, dyn.use_elu, dyn.loop_consts(), GAMMA)
            status = arrays['status'].cpu().numpy()
            action = action.cpu().numpy()
        if status.any():
            m = int(np.flatnonzero(status)[0])
            raise RuntimeError('device search: tree %d stopped with status %d (%s); the host arrays are as before the search, the state '
                               'pool is not: the iterations that ran have written child states into it' % (
                                   m, status[m], {1: 'out of slots', 2: 'an index check failed'}.get(int(status[m]), 'unknown')))
        f.from_device(arrays)
        self.timing = {'host': 0.0, 'device': time.perf_counter() - t0}
        return [int(a) for a in action]

    def _expand_fused(self, env, acts_all, app):
        from .. import ops
        dyn, f = env.dyn, self.forest
        dev = f.z.device
        emb_w, emb_b, gnn, rh = self._fused_weights(env)
        acts = torch.from_numpy(acts_all.astype(np.int32)).to(dev)                    # every iteration's actions, one upload
        consts, elu = dyn.loop_consts(), dyn.use_elu

        def expand(i, leaf, child, len_s):
            idx = torch.from_numpy(np.stack([leaf, child, len_s]).astype(np.int32)).to(dev)
            q = ops.plan_expand(f.z, idx[0], idx[1], idx[2], app, acts[i], emb_w, emb_b, gnn, rh, self.max_rollout, 2, elu, consts, GAMMA)
            return q.double().cpu().numpy()
        return expand

    def _expand_composed(self, env, acts_all, app):
        """the reference's run_mcts body (mcts_stove.py:104-137) on the pool: two Stove.rollout calls per iteration"""
        M, A, D, f = self.num_mcts, self.actions, self.max_rollout, self.forest
        dev = f.z.device
        rows = torch.arange(M, device=dev)
        app_t = tile(app, 0, A) if app is not None else None

        def expand(i, leaf, child, len_s):
            z = f.z[rows, torch.from_numpy(leaf).to(dev)]
            expansion_actions = multi_one_hot(range(A), A).view(A, 1, A).repeat(M, 1, 1).to(dev)
            new_zs, r = env.rollout(tile(z, 0, A), num=1, actions=expansion_actions, appearance=app_t)
            random_rollout_actions = multi_one_hot(acts_all[i].reshape(-1), A).view(M * A, 2 * D, A).to(dev)
            _, r_rollout = env.rollout(new_zs[:, -1], num=2 * D, actions=random_rollout_actions, appearance=app_t)
            slots = torch.from_numpy(child[:, None] + np.arange(A)).to(dev)
            f.z[rows[:, None], slots] = new_zs[:, -1].view(M, A, *new_zs.shape[2:])
            rs = r.reshape(M, A).cpu().numpy()
            rr = r_rollout.reshape(M, A, 2 * D).cpu().numpy()
            return discounted_values(rs, rr, len_s, D, GAMMA)
        return expand


def initialize_img(envs, steps=8, res=32):
    num_parallel_envs = len(envs)
    img = np.zeros((num_parallel_envs, steps, res, res, 3))
    for i in range(num_parallel_envs):
        for j in range(steps):
            ret_img, _, _, _ = envs[i].step(0)
            img[i, j] = ret_img
    actions = multi_one_hot([0] * steps * num_parallel_envs, 9)
    actions = actions.view(num_parallel_envs, steps, 9)
    return img, actions


def update_buffer(img, new_img, action, new_action):
    img[:, :-1] = img[:, 1:]
    img[:, -1] = new_img
    new_action = multi_one_hot(new_action, 9)
    action[:, :-1] = action[:, 1:]
    action[:, -1] = new_action
    return img, action


def run_mcts_model(img, model, actions, num_parallel_envs=100, mcts_steps=100, max_rollout_depth=10):
    """img (envs, time, width, height, channels): the last frames of every environment; actions (envs, time, 9) one-hot: the actions
    taken -> the next action of every environment, by `mcts_steps` expansions per tree on `model`."""
    return plan_on_model(img, model, actions, num_parallel_envs, mcts_steps, max_rollout_depth)


def plan_on_model(img, model, actions, num_parallel_envs=100, mcts_steps=100, max_rollout_depth=10, fused=None, device_trees=False,
                  fused_widths=None):
    """run_mcts_model (the reference's surface, whose parameter list stays the reference's) with the search's switches as arguments:
    `fused` as BatchedMCTSHandler.run_mcts takes it, `device_trees` and `fused_widths` as the handler's attributes of those names
    (fused_widths None: FUSED_WIDTHS)."""
    return plan_on_frames(encode_img(img), model, actions, num_parallel_envs, mcts_steps, max_rollout_depth, fused, device_trees, fused_widths)


def plan_on_frames(x, model, actions, num_parallel_envs=100, mcts_steps=100, max_rollout_depth=10, fused=None, device_trees=False,
                   fused_widths=None):
    """plan_on_model on frames already in the model's layout: x (envs, time, channels, width, height) float32, on any device (frames
    rendered on the model's device reach it without a host round trip)."""
    dev = next(model.parameters()).device
    with torch.no_grad():
        _, prop_dict, _ = model(x.to(dev), 0, actions=actions.to(dev), pretrain=False)
        apps = prop_dict['obj_appearances']
        all_mcts = [MCTS(apps[env:env + 1, -1] if apps is not None else None, prop_dict['z'][env:env + 1, -1],
                         max_rollout_depth=max_rollout_depth) for env in range(num_parallel_envs)]
        mcts = BatchedMCTSHandler(all_mcts, apps[:, -1] if apps is not None else None, action_space=9,
                                  max_rollout_depth=max_rollout_depth)
        mcts.device_trees = device_trees
        if fused_widths is not None:
            mcts.fused_widths = tuple(fused_widths)
        all_actions = mcts.run_mcts(model, mcts_steps, fused=fused)
    return all_actions
