"""A batch of avoidance / billiards environments stepped and rendered together: the environment side of closed-loop planning
(stove_amd/mcts/play.py).

`BatchedAvoidance` holds M environments that share N, res, granularity, hw, t, friction and the flags as arrays x, v (M, N, 2),
r, m (M, N) in float64.  On the host (device=None) a step is numpy, vectorised over the environments with ELEMENTWISE ufuncs only,
in the operation order of stove_amd/csrc/env_step.h -- which restates PhysicsEnv.step + BillardsEnv.simulate_physics +
AvoidanceTask.step of envs.py with plain sqrt(a a + b b) norms and a c + b d dot products where envs.py calls BLAS.  On a GPU the
arrays are tensors and a step is one ops.env_step call (stove_env_step, csrc/env.hip), which reproduces the host arithmetic bit for
bit in x, v and collisions; frames agree to one float32 ulp (exp is a library call on either side).  Gravity has no actions and
stays on the host (envs.GravityEnv)."""
import numpy as np
import torch

from . import envs as _envs

ACTIONS = 9
_SHARED = ('n', 'res', 'granularity', 'hw', 't', 'friction', 'drift', 'use_colors', 'action_force')


def _directions():
    s = 1.0 / np.sqrt(2.0)
    return np.array([[0., 0.], [1., 0.], [0., 1.], [s, s], [-1., 0.], [0., -1.], [-s, -s], [-s, s], [s, -s]])


class BatchedAvoidance:
    """M reference-style avoidance environments (BillardsEnv(n, hw, r, res, seed) under AvoidanceTask(action_force)), one per seed."""

    def __init__(self, seeds, n=3, hw=10, r=1., res=32, granularity=5, action_force=.6, device=None, **env_kwargs):
        tasks = [_envs.AvoidanceTask(_envs.BillardsEnv(n=n, hw=hw, r=r, res=res, granularity=granularity, seed=s, **env_kwargs),
                                     action_force=action_force) for s in seeds]
        self._take(tasks, device)

    @classmethod
    def from_tasks(cls, tasks, device=None):
        """the current state and settings of a list of AvoidanceTask (copied: the tasks are left alone)"""
        self = cls.__new__(cls)
        self._take(tasks, device)
        return self

    def _take(self, tasks, device):
        tasks = list(tasks)
        if not tasks:
            raise ValueError('BatchedAvoidance needs at least one environment')
        cfgs = []
        for task in tasks:
            e = task.env
            if not isinstance(e, _envs.BillardsEnv):
                raise ValueError('BatchedAvoidance steps billiards environments; %s stays on the host' % type(e).__name__)
            cfgs.append(dict(n=int(e.n), res=int(e.res), granularity=int(e.internal_steps), hw=float(e.hw), t=float(e.t),
                             friction=float(e.fric_coeff), drift=bool(e.drift), use_colors=bool(e.use_colors),
                             action_force=float(task.action_force)))
        for k in _SHARED:
            if any(c[k] != cfgs[0][k] for c in cfgs):
                raise ValueError('environments of one batch share %s; got %s' % (k, sorted({c[k] for c in cfgs})))
        for k, val in cfgs[0].items():
            setattr(self, k, val)
        if not 1 <= self.n <= 6:
            raise ValueError('BatchedAvoidance holds 1 .. 6 objects per environment, not %d' % self.n)
        self.M = len(tasks)
        self.device = None
        self.x = np.stack([np.array(t.env.x, dtype=np.float64).reshape(self.n, 2) for t in tasks])
        self.v = np.stack([np.array(t.env.v, dtype=np.float64).reshape(self.n, 2) for t in tasks])
        self.r = np.stack([np.array(t.env.r, dtype=np.float64).reshape(self.n) for t in tasks])
        self.m = np.stack([np.array(t.env.m, dtype=np.float64).reshape(self.n) for t in tasks])
        self.status = np.zeros(self.M, dtype=np.int32)
        if device is not None:
            self.to(device)

    # ------------------------------------------------------------------------------------------------ where the batch lives
    def to(self, device):
        """move the state to `device` (a CUDA device: steps run stove_env_step) or back to numpy (None or 'cpu')"""
        dev = None if device is None else torch.device(device)
        if dev is not None and dev.type == 'cpu':
            dev = None
        for name in ('x', 'v', 'r', 'm', 'status'):
            a = getattr(self, name)
            if isinstance(a, torch.Tensor):
                a = a.cpu().numpy()
            setattr(self, name, a if dev is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev))
        self.device = dev
        return self

    def _host(self, name):
        a = getattr(self, name)
        return a.cpu().numpy() if isinstance(a, torch.Tensor) else a

    def state(self):
        """(M, N, 4): positions and velocities, where the batch lives"""
        if self.device is None:
            return np.concatenate([self.x, self.v], axis=2)
        return torch.cat([self.x, self.v], dim=2)

    def tasks(self):
        """-> a fresh list of AvoidanceTask carrying the current state (their random streams are new: a step draws nothing)"""
        x, v, r, m = (self._host(k) for k in ('x', 'v', 'r', 'm'))
        hw = int(self.hw) if float(self.hw).is_integer() else self.hw
        out = []
        for e in range(self.M):
            # (built with pin-point balls so that the constructor's rejection sampling of a start passes at once; then this state)
            env = _envs.BillardsEnv(n=self.n, r=1e-9, m=1., hw=hw, granularity=self.granularity, res=self.res, t=self.t,
                                    friction_coefficient=self.friction, seed=0, use_colors=self.use_colors, drift=self.drift)
            env.r, env.m = r[e].reshape(self.n, 1).copy(), m[e].reshape(self.n, 1).copy()
            env.x, env.v = x[e].copy(), v[e].copy()
            m0 = env.m[0].copy()
            task = _envs.AvoidanceTask(env, action_force=self.action_force)
            env.m[0] = m0          # (the constructor set 10000; this batch's mass is what was copied)
            out.append(task)
        return out

    # ------------------------------------------------------------------------------------------------ one step
    def step(self, actions, render=True):
        """actions (M,) indices into AvoidanceTask.action_selection, or None (plain billiards) -> (frames (M, 3, res, res) float32 in
        the model's layout -- None with render=False --, reward (M,) = -collisions).  self.status (M,): 2 where the action index was
        outside [0, 9) -- that environment is left untouched (its frame row is not written: zeros on the host)."""
        if self.device is not None:
            from .. import ops
            if actions is not None:
                actions = torch.as_tensor(actions).to(device=self.device, dtype=torch.int32).contiguous()
            frames, collisions, self.status = ops.env_step(self.x, self.v, self.r, self.m, actions, self.granularity, self.res, self.hw, self.t,
                                                           self.friction, self.action_force, use_colors=self.use_colors, drift=self.drift,
                                                           render=render)
            return frames, -collisions
        M = self.M
        ok = np.ones(M, dtype=bool)
        if actions is not None:
            actions = np.asarray(actions).astype(np.int64).reshape(M)
            ok = (actions >= 0) & (actions < ACTIONS)
        self.status = np.where(ok, 0, 2).astype(np.int32)
        collisions = np.zeros(M, dtype=np.int32)
        frames = np.zeros((M, 3, self.res, self.res), dtype=np.float32) if render else None
        if ok.any():
            x, v = self.x[ok], self.v[ok]
            collisions[ok] = self._step_rows(x, v, self.r[ok], self.m[ok], None if actions is None else actions[ok])
            self.x[ok], self.v[ok] = x, v
            if render:
                frames[ok] = self._draw(x, self.r[ok])
        return frames, -collisions

    def _step_rows(self, x, v, r, m, actions):
        """env_step.h: step + collide on rows (K, N, 2), in place -> collisions (K,).  A branch of the header is a mask here."""
        N, t, hw, fric = self.n, self.t, self.hw, self.friction
        acting = actions is not None
        if acting:
            v[:, 0] = _directions()[actions] * self.action_force * t
        eps = 1.0 / float(self.granularity)
        te = t * eps
        dt = eps * t
        hit = np.zeros(x.shape[0], dtype=bool)
        for _ in range(self.granularity):
            x += te * v
            v -= fric * m[:, :, None] * v * t * eps
            for i in range(N):
                ri = r[:, i]
                for ax in range(2):
                    nxt = x[:, i, ax] + v[:, i, ax] * dt
                    low = nxt < ri
                    high = ~low & (nxt > hw - ri)
                    x[:, i, ax] = np.where(low, ri, np.where(high, hw - ri, x[:, i, ax]))
                    v[:, i, ax] = np.where(low | high, -v[:, i, ax], v[:, i, ax])
            if self.drift:
                continue
            for i in range(N):
                for j in range(i):
                    g = (x[:, i] + v[:, i] * t * eps) - (x[:, j] + v[:, j] * t * eps)
                    gap = np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1])
                    touch = gap < r[:, i] + r[:, j]
                    if not touch.any():
                        continue
                    controlled = acting and j == 0
                    if controlled:
                        hit |= touch
                    w = x[:, i] - x[:, j]
                    with np.errstate(divide='ignore', invalid='ignore'):          # (rows that do not touch are computed and dropped)
                        w = w / np.sqrt(w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1])[:, None]
                        v_i = w[:, 0] * v[:, i, 0] + w[:, 1] * v[:, i, 1]
                        v_j = w[:, 0] * v[:, j, 0] + w[:, 1] * v[:, j, 1]
                        if controlled:
                            v_j = np.zeros_like(v_j)
                        m1, m2 = m[:, i], m[:, j]
                        new_v_j = (2.0 * m1 * v_i + v_j * (m2 - m1)) / (m1 + m2)
                        new_v_i = new_v_j + (v_j - v_i)
                        vi = v[:, i] + w * (new_v_i - v_i)[:, None]
                        vj = v[:, j] + w * (new_v_j - v_j)[:, None]
                    if controlled:
                        vj = np.zeros_like(vj)
                    v[:, i] = np.where(touch[:, None], vi, v[:, i])
                    v[:, j] = np.where(touch[:, None], vj, v[:, j])
        return hit.astype(np.int32)

    def _centres(self):
        res = self.res
        return (0.5 / float(res) + np.arange(res, dtype=np.float64) * (1.0 / float(res))) * self.hw

    def _draw(self, x, r):
        """env_step.h: pixel on rows (K, N, 2) -> (K, 3, res, res) float32; pixel (a, b) sits at (centre[b], centre[a])"""
        c = self._centres()
        acc = np.zeros((x.shape[0], 3, self.res, self.res))
        for i in range(self.n):
            d0 = c[None, None, :] - x[:, i, 0, None, None]
            d1 = c[None, :, None] - x[:, i, 1, None, None]
            u = (d0 * d0 + d1 * d1) / (r[:, i] * r[:, i])[:, None, None]
            u2 = u * u
            blob = np.exp(-(u2 * u2))
            for ch in range(3):
                if (_envs.BALL_COLOURS[i, ch] if self.use_colors else ch == i % 3):
                    acc[:, ch] = acc[:, ch] + blob
        return np.where(acc > 1.0, 1.0, acc).astype(np.float32)

    def frames(self):
        """the frame of the current state (M, 3, res, res) float32 on the host, whatever the last step rendered"""
        return self._draw(self._host('x'), self._host('r'))
