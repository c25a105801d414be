"""Whole training sequences synthesised together: the batched counterpart of envs.synth_sequences and of the reference's data-file
command (model/envs/envs.py: generate_fitting_run, generate_data, generate_billiards_w_actions).

A step of an environment draws nothing, so all randomness of a sequence -- its start and, with actions, its action row -- is known
before it starts: `draw_starts` runs the constructors and the action policy exactly as envs.synth_sequences does and steps nothing.
`BatchedSequences` then simulates all B sequences together in numpy, vectorised over sequences with ELEMENTWISE ufuncs only, in the
operation order of stove_amd/csrc/env_step.h (billiards: BatchedAvoidance._step_rows / _draw) and stove_amd/csrc/env_gravity.h
(gravity: _gravity_rows, which restates PhysicsEnv.step + GravityEnv.simulate_physics with sqrt(a a + b b) norms and d * d * d cubes
where envs.py calls BLAS and pow).  On a GPU the same sequences are one ops.env_sequences call (stove_env_sequences,
csrc/env_sequences.hip), which reproduces the numpy states bit for bit; frames agree to one float32 ulp.

`draw_starts_counter` is a second, opt-in way to draw the same things (starts='counter'): a counter-based stream with a specification
of its own (csrc/env_draw.h) that a GPU reproduces bit for bit in one ops.env_draw_starts launch (stove_env_draw_starts,
csrc/env_draw.hip), so that nothing of a sequence is computed on the host.  The same distributions as draw_starts', other numbers."""
import os
import pickle

import numpy as np
import torch

from . import envs as _envs
from .batched import ACTIONS, BatchedAvoidance

G, SOFTENING, PULL = 0.5, 1e-5, 0.001


def _config(preset):
    """a preset's name, or a dict in the manner of envs.ENV_PRESETS (cls and the constructor's arguments)"""
    return dict(_envs.ENV_PRESETS[preset]) if isinstance(preset, str) else dict(preset)


def _make(preset, seed, res=None):
    if isinstance(preset, str):
        return _envs.make_env(preset, seed, res)
    cfg = _config(preset)
    if res is not None:
        cfg['res'] = int(res)
    cls = {'billiards': _envs.BillardsEnv, 'gravity': _envs.GravityEnv}[cfg.pop('cls')]
    return cls(seed=seed, **cfg)


def draw_starts(preset, n_seq, t_len, seed0=0, with_actions=None, res=None):
    """Everything random of sequences seed0 .. seed0 + n_seq - 1, drawn as envs.synth_sequences draws it: the constructor's start and,
    with actions, m[0] = 10000, uniform(0.2, 0.3), the MonteCarloActionPolicy constructor and t_len calls of next().  No environment is
    stepped.  -> dict(x0, v0 (B, N, 2), r, m (B, N) float64, actions (B, T) int32 or None, settings: the shared settings)"""
    with_actions = (preset == 'avoidance') if with_actions is None else with_actions
    x0, v0, r, m, acts, settings = [], [], [], [], [], None
    for i in range(n_seq):
        env = _make(preset, seed0 + i, res)
        if with_actions:
            task = _envs.AvoidanceTask(env, 4, greyscale=False, action_force=0.6)
            policy = _envs.MonteCarloActionPolicy(9, env.rng.uniform(0.2, 0.3), rng=env.rng)
            acts.append([policy.next() for _ in range(t_len)])
        n = int(env.n)
        x0.append(np.array(env.x, dtype=np.float64).reshape(n, 2))
        v0.append(np.array(env.v, dtype=np.float64).reshape(n, 2))
        r.append(np.array(env.r, dtype=np.float64).reshape(n))
        m.append(np.array(env.m, dtype=np.float64).reshape(n))
        if settings is None:
            settings = dict(n=n, res=int(env.res), granularity=int(env.internal_steps), hw=float(env.hw), t=float(env.t),
                            friction=float(env.fric_coeff), drift=bool(getattr(env, 'drift', False)), use_colors=bool(env.use_colors),
                            action_force=float(task.action_force) if with_actions else 0.6, gravity=isinstance(env, _envs.GravityEnv))
    if settings is None:          # (no sequence: the settings of the preset, from a throw-away environment)
        settings = draw_starts(preset, 1, 1, seed0, with_actions, res)['settings']
    n = settings['n']
    if with_actions and settings['gravity']:
        raise ValueError('gravity takes no actions')
    return dict(x0=np.array(x0, dtype=np.float64).reshape(n_seq, n, 2), v0=np.array(v0, dtype=np.float64).reshape(n_seq, n, 2),
                r=np.array(r, dtype=np.float64).reshape(n_seq, n), m=np.array(m, dtype=np.float64).reshape(n_seq, n),
                actions=np.array(acts, dtype=np.int32).reshape(n_seq, t_len) if with_actions else None, settings=settings)


# ---- the counter-based stream (stove_amd/csrc/env_draw.h): a second, opt-in random stream.  The same distributions as draw_starts', other
# numbers: RandomState's normals go through libm's log, which a device cannot reproduce, so this stream has a specification of its own --
# Philox4x32-10 counters, integer arithmetic up to the uniform double, then + - * / sqrt in env_draw.h's order with its own logarithm.
# Everything below is elementwise numpy on arrays over sequences (and blocks of attempts), so host, driver and kernel agree bit for bit.
START_TRIES = 1 << 20
_POSITIONS, _NORMALS, _SCALARS, _ACTION_STREAM = 0, 1, 2, 3
_GRAVITY_TRIES, _NORMAL_TRIES = 1000, 64
_MASK32 = np.uint64(0xffffffff)


def _philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint64 arrays that hold 32-bit words -> the four output words"""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*[np.asarray(a, dtype=np.uint64) for a in (c0, c1, c2, c3, k0, k1)])
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _MASK32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _MASK32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _MASK32, (k1 + np.uint64(0xBB67AE85)) & _MASK32
    return c0, c1, c2, c3


def _uniform(a, b):
    """numpy's double from two 32-bit words: ((a >> 5) 2^26 + (b >> 6)) / 2^53"""
    return ((a >> np.uint64(5)).astype(np.float64) * 67108864.0 + (b >> np.uint64(6)).astype(np.float64)) / 9007199254740992.0


def _block(seed, stream, attempt, index):
    """the two uniforms of block `index` of `attempt` of `stream` for the seeds `seed` (uint64), broadcast"""
    seed = np.asarray(seed, dtype=np.uint64)
    w = _philox(index, attempt, 0, stream, seed & _MASK32, seed >> np.uint64(32))
    return _uniform(w[0], w[1]), _uniform(w[2], w[3])


def log_pos(x):
    """env_draw.h's log_pos on an array of positive normal doubles"""
    bits = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    e = ((bits >> np.uint64(52)) & np.uint64(0x7ff)).astype(np.int64) - 1023
    m = ((bits & np.uint64(0x000fffffffffffff)) | np.uint64(0x3ff0000000000000)).view(np.float64)
    big = m >= 1.4142135623730951
    m = np.where(big, m * 0.5, m)
    e = e + big
    s = (m - 1.0) / (m + 1.0)
    z = s * s
    p = np.full_like(s, 1.0 / 23.0)
    for k in (21.0, 19.0, 17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0, 1.0):
        p = p * z + 1.0 / k
    de = e.astype(np.float64)
    return de * 6.93147180369123816490e-01 + (2.0 * s * p + de * 1.90821492927058770002e-10)


def _normal(seed, j):
    """standard normal number j (broadcast against the seeds): the polar method, try t on block (j, t)"""
    seed, j = np.broadcast_arrays(np.asarray(seed, dtype=np.uint64), np.asarray(j, dtype=np.uint64))
    out, todo = np.zeros(seed.shape), np.ones(seed.shape, dtype=bool)
    for t in range(_NORMAL_TRIES):
        if not todo.any():
            break
        u, w = _block(seed, _NORMALS, t, j)
        a, c = 2.0 * u - 1.0, 2.0 * w - 1.0
        s = a * a + c * c
        ok = todo & (s < 1.0) & (s > 0.0)
        safe = np.where(ok, s, 0.5)
        out = np.where(ok, a * np.sqrt(-2.0 * log_pos(safe) / safe), out)
        todo = todo & ~ok
    return out


def _attempts(seed, ks, r, hw, gravity):
    """attempts `ks` (K,) of the sequences `seed` (P,), radii r (P, N) -> x (P, K, N, 2), good (P, K): env_draw.h's *_attempt"""
    N = r.shape[1]
    u, w = _block(seed[:, None, None], _POSITIONS, ks[None, :, None], np.arange(N)[None, None, :])
    if gravity:
        x = np.stack([u * 0.9 * hw / 2.0 + hw / 2.0, w * 0.9 * hw / 2.0 + hw / 2.0], axis=-1)
        good = np.ones(x.shape[:2], dtype=bool)
    else:
        x = np.stack([u * hw / 2.0 + hw / 4.0, w * hw / 2.0 + hw / 4.0], axis=-1)
        rr = r[:, None, :, None]
        good = ((x - rr >= 0.0) & (x + rr <= hw)).all((2, 3))
    for i in range(1, N):
        for j in range(i):
            a, c = x[:, :, i, 0] - x[:, :, j, 0], x[:, :, i, 1] - x[:, :, j, 1]
            d = np.sqrt(a * a + c * c)
            good = good & ((d > hw / 3.0) if gravity else (d >= (r[:, i] + r[:, j])[:, None]))
    return x, good


def _preset_settings(preset, with_actions, res):
    """draw_starts' settings, radii and masses of one sequence from the preset alone, by the constructors' defaults: no environment is
    made -> (settings, r (N,), m (N,), the constructor's init_v_factor or None)"""
    cfg = _config(preset)
    gravity = cfg['cls'] == 'gravity'
    n = int(cfg.get('n', 3))
    use_colors = cfg.get('use_colors', False if gravity else None)
    settings = dict(n=n, res=int(cfg.get('res', 32) if res is None else res), granularity=int(cfg.get('granularity', 5)),
                    hw=float(cfg.get('hw', 10)), t=float(cfg.get('t', 1.0)), friction=float(cfg.get('friction_coefficient', 0.0)),
                    drift=bool(cfg.get('drift', False)), use_colors=bool(n >= 3 if use_colors is None else use_colors), action_force=0.6,
                    gravity=gravity)
    r = np.array(np.broadcast_to(np.asarray(cfg.get('r', 1.0), dtype=np.float64).reshape(-1), (n,)))
    m = np.array(np.broadcast_to(np.asarray(cfg.get('m', 1.0), dtype=np.float64).reshape(-1), (n,)))
    if with_actions:
        m[0] = 10000.0          # (AvoidanceTask: the controlled ball is quasi-static)
    return settings, r, m, cfg.get('init_v_factor', 0.18 if gravity else None)


def draw_starts_counter(preset, n_seq, t_len, seed0=0, with_actions=None, res=None, max_tries=START_TRIES):
    """draw_starts on the counter-based stream: the numpy specification of stove_env_draw_starts (csrc/env_draw.h, csrc/env_draw.hip).
    Sequence i is a pure function of its seed seed0 + i.  -> draw_starts' dict plus tries (B,) int32, the index of the attempt taken
    plus one, and status (B,) int32: 1 where none of max_tries billiards attempts was good (zero x0 and v0 rows, tries = max_tries)."""
    with_actions = (preset == 'avoidance') if with_actions is None else with_actions
    settings, r1, m1, factor = _preset_settings(preset, with_actions, res)
    gravity, n, hw = settings['gravity'], settings['n'], settings['hw']
    if with_actions and gravity:
        raise ValueError('gravity takes no actions')
    B, T, max_tries = int(n_seq), int(t_len), int(max_tries)
    if max_tries < 1 or max_tries > 0x7fffffff or not 1 <= n <= 6:
        raise ValueError('draw_starts_counter: max_tries must be in [1, 2^31) and n in 1 .. 6')
    seed = (np.uint64(int(seed0) & 0xffffffffffffffff) + np.arange(B, dtype=np.uint64))
    r, m = np.tile(r1, (B, 1)), np.tile(m1, (B, 1))
    x0, v0 = np.zeros((B, n, 2)), np.zeros((B, n, 2))
    tries, status = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    limit = _GRAVITY_TRIES if gravity else max_tries
    todo, base, width = np.arange(B), 0, 64
    while todo.size and base < limit:
        ks = np.arange(base, min(base + width, limit), dtype=np.uint64)
        x, good = _attempts(seed[todo], ks, r[todo], hw, gravity)
        found, first = good.any(1), good.argmax(1)
        x0[todo[found]] = x[found, first[found]]
        tries[todo[found]] = (base + first[found] + 1).astype(np.int32)
        if gravity and base + ks.size == limit:         # (GravityEnv.init_x keeps its last attempt)
            x0[todo[~found]] = x[~found, -1]
            tries[todo[~found]] = limit
            found = np.ones_like(found)
        todo, base, width = todo[~found], base + ks.size, min(2 * width, 8192)
    status[todo], tries[todo] = 1, max_tries
    ok = status == 0
    if gravity:
        c = x0[:, 0]
        for i in range(1, n):
            c = c + x0[:, i]
        c = c / float(n)
        sign = np.where(_block(seed, _SCALARS, 0, 0)[0] < 0.5, -1.0, 1.0)
        for i in range(n):
            d = x0[:, i] - c
            with np.errstate(divide='ignore', invalid='ignore'):          # (one ball sits in its own centre: 0 / 0, as in envs.py)
                d = d / np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])[:, None]
            v0[:, i, 0] = sign * d[:, 1] * (factor + 0.13 * _normal(seed, 2 * i))
            v0[:, i, 1] = -sign * d[:, 0] * (factor + 0.13 * _normal(seed, 2 * i + 1))
    else:
        z = _normal(seed[:, None], np.arange(2 * n)[None, :])
        ss = np.zeros(B)
        for j in range(2 * n):
            ss = ss + z[:, j] * z[:, j]
        v = z / np.sqrt(ss)[:, None] * 0.5
        if factor is not None and factor > 0.0:
            lo = 1.0 / factor
            v = v * (lo + (factor - lo) * _block(seed, _SCALARS, 0, 0)[0])[:, None]
        v0[ok] = v.reshape(B, n, 2)[ok]
    actions = None
    if with_actions:
        u, w = _block(seed, _ACTION_STREAM, 0, 0)
        p, cur = 0.2 + 0.1 * u, (9.0 * w).astype(np.int64)
        u, w = _block(seed[:, None], _ACTION_STREAM, 1, np.arange((T + 1) // 2)[None, :])
        us = np.stack([u, w], axis=-1).reshape(B, -1)[:, :T]
        other, stay = p / 8.0, 1.0 - p
        actions = np.zeros((B, T), dtype=np.int32)
        for s in range(T):
            acc, pick, found = np.zeros(B), np.full(B, ACTIONS - 1, dtype=np.int64), np.zeros(B, dtype=bool)
            for a in range(ACTIONS):
                acc = acc + np.where(cur == a, stay, other)
                hit = ~found & (us[:, s] < acc)
                pick, found = np.where(hit, a, pick), found | hit
            cur = pick
            actions[:, s] = cur
    return dict(x0=x0, v0=v0, r=r, m=m, actions=actions, settings=settings, tries=tries, status=status)


class BatchedSequences(BatchedAvoidance):
    """The numpy specification of stove_env_sequences: B sequences from draw_starts' arrays, all stepped together."""

    def __init__(self, starts):
        for k, val in starts['settings'].items():
            setattr(self, k, val)
        self.M = starts['x0'].shape[0]
        self.device = None
        self.x, self.v = starts['x0'].copy(), starts['v0'].copy()
        self.r, self.m = starts['r'].copy(), starts['m'].copy()
        self.actions = starts['actions']
        self.status = np.zeros(self.M, dtype=np.int32)

    def _gravity_rows(self, x, v, m):
        """env_gravity.h: step on rows (K, N, 2), in place"""
        N, t, hw, fric = self.n, self.t, self.hw, self.friction
        eps = 1.0 / float(self.granularity)
        te = t * eps
        mid = hw / 2.0
        for _ in range(self.granularity):
            x += te * v
            s = m[:, 0, None] * x[:, 0]
            sm = m[:, 0].copy()
            for i in range(1, N):
                s = s + m[:, i, None] * x[:, i]
                sm = sm + m[:, i]
            x += (hw / 2.0 - s / sm[:, None])[:, None, :]
            v -= fric * m[:, :, None] * v * t * eps
            for i in range(N):
                f = np.zeros((x.shape[0], 2))
                for j in range(N):
                    if j == i:
                        continue
                    a = x[:, j] - x[:, i]
                    d = np.sqrt(a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + SOFTENING
                    cube = d * d * d
                    g = G * m[:, j] * m[:, i]
                    f = f - g[:, None] * (x[:, i] - x[:, j]) / cube[:, None]
                c = mid - x[:, i]
                nrm = np.sqrt(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1])
                with np.errstate(divide='ignore', invalid='ignore'):          # (a ball exactly in the middle: 0 / 0, as in envs.py)
                    f = f + PULL * (c * c * c) / nrm[:, None]
                f = np.where(f < -1.0, -1.0, np.where(f > 1.0, 1.0, f))
                v[:, i] = v[:, i] + (f / m[:, i, None]) * t * eps

    def run(self, t_len, render=True):
        """-> dict(y (B, T, N, 4) float64, X (B, T, 3, res, res) float32 or None, collisions (B, T) int32, in_bounds (B,) int32, status
        (B,) int32).  A sequence with an action index outside [0, 9) gets status 2 and zero rows."""
        B, N, T = self.M, self.n, int(t_len)
        ok = np.ones(B, dtype=bool)
        acts = None
        if self.actions is not None:
            acts = np.asarray(self.actions).astype(np.int64).reshape(B, T)
            ok = ((acts >= 0) & (acts < ACTIONS)).all(1)
        self.status = np.where(ok, 0, 2).astype(np.int32)
        y = np.zeros((B, T, N, 4))
        X = np.zeros((B, T, 3, self.res, self.res), dtype=np.float32) if render else None
        collisions = np.zeros((B, T), dtype=np.int32)
        in_bounds = np.zeros(B, dtype=np.int32)
        if ok.any():
            x, v, r, m = self.x[ok], self.v[ok], self.r[ok], self.m[ok]
            count = np.zeros(x.shape[0], dtype=np.int32)
            for s in range(T):
                if self.gravity:
                    self._gravity_rows(x, v, m)
                else:
                    collisions[ok, s] = self._step_rows(x, v, r, m, None if acts is None else acts[ok, s])
                y[ok, s] = np.concatenate([x, v], axis=2)
                count += ((x > 0.0) & (x < self.hw)).sum((1, 2)).astype(np.int32)
                if render:
                    X[ok, s] = self._draw(x, r)
            in_bounds[ok] = count
            self.x[ok], self.v[ok] = x, v
        return dict(y=y, X=X, collisions=collisions, in_bounds=in_bounds, status=self.status)


def accepted(in_bounds, t_len, n):
    """generate_fitting_run's rule: a run is kept iff its balls' coordinates, counted per step as a fraction of the 2 n, sum to more
    than t_len - t_len / 100 -> boolean mask"""
    if isinstance(in_bounds, torch.Tensor):
        in_bounds = in_bounds.cpu().numpy()
    return np.asarray(in_bounds) / (2 * n) > (t_len - t_len / 100)


def _device(device):
    dev = None if device is None else torch.device(device)
    return None if dev is not None and dev.type == 'cpu' else dev


def run_starts(starts, t_len, device=None, render=True):
    """draw_starts' arrays simulated: on the host by BatchedSequences, on a GPU by one ops.env_sequences call (y, X, collisions,
    in_bounds, status then are device tensors; start arrays that already are tensors on that device are used where they lie)
    -> BatchedSequences.run's dict"""
    dev = _device(device)
    if dev is None:
        return BatchedSequences(starts).run(t_len, render=render)
    from .. import ops
    s = starts['settings']
    up = lambda a: a if a is None or isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = ops.env_sequences(up(starts['x0']), up(starts['v0']), up(starts['r']), up(starts['m']), up(starts['actions']), t_len, s['granularity'],
                            s['res'], s['hw'], s['t'], s['friction'], s['action_force'], use_colors=s['use_colors'], drift=s['drift'],
                            gravity=s['gravity'], render=render)
    return dict(y=out['y'], X=out['frames'], collisions=out['collisions'], in_bounds=out['in_bounds'], status=out['status'])


def draw_starts_device(preset, n_seq, t_len, seed0=0, with_actions=None, res=None, max_tries=START_TRIES, device='cuda'):
    """draw_starts_counter on a GPU: one ops.env_draw_starts launch -> its dict with x0, v0, r, m, actions, tries and status as device
    tensors.  Only the preset's radii and masses, the same for every sequence, are uploaded."""
    from .. import ops
    with_actions = (preset == 'avoidance') if with_actions is None else with_actions
    settings, r1, m1, factor = _preset_settings(preset, with_actions, res)
    if with_actions and settings['gravity']:
        raise ValueError('gravity takes no actions')
    dev = torch.device(device)
    r = torch.from_numpy(r1).to(dev).repeat(int(n_seq), 1)
    m = torch.from_numpy(m1).to(dev).repeat(int(n_seq), 1)
    out = ops.env_draw_starts(r, t_len, seed0, settings['hw'], gravity=settings['gravity'], v_factor=factor or 0.0, with_actions=with_actions,
                              max_tries=max_tries)
    return dict(x0=out['x0'], v0=out['v0'], r=r, m=m, actions=out['actions'], settings=settings, tries=out['tries'], status=out['status'])


def synth_sequences_batched(preset, n_seq, t_len, seed0=0, with_actions=None, res=None, device=None, starts='host', start_tries=START_TRIES):
    """envs.synth_sequences with all sequences simulated together -> its dict (X (B,T,3,res,res) f32, y (B,T,n,4) f64 [, action (B,T,9),
    reward (B,T,1)]) plus in_bounds (B,).  device=None: the numpy specification, numpy arrays; a GPU device: one ops.env_sequences
    call, X, y and in_bounds device tensors (action and reward stay on the host, built from the action rows).
    starts='host': the starts and action rows are envs.synth_sequences' own, drawn by draw_starts.  starts='counter': the counter-based
    stream (draw_starts_counter: other numbers, the same distributions) -- in numpy with device=None, on a GPU one ops.env_draw_starts
    launch in front of the ops.env_sequences launch, nothing of a sequence computed on the host.  A sequence for which none of
    start_tries attempts gave a start runs from zero rows and is no data: generate_runs counts it as rejected."""
    return _synth_batched(preset, n_seq, t_len, seed0, with_actions, res, device, starts, start_tries)[0]


def _synth_batched(preset, n_seq, t_len, seed0, with_actions, res, device, starts, start_tries):
    """synth_sequences_batched -> (its dict, the starts' status (B,) -- host array or device tensor -- or None with starts='host')"""
    if starts not in ('host', 'counter'):
        raise ValueError("starts must be 'host' or 'counter', not %r" % (starts,))
    dev = _device(device)
    if starts == 'host':
        drawn = draw_starts(preset, n_seq, t_len, seed0, with_actions, res)
    elif dev is None:
        drawn = draw_starts_counter(preset, n_seq, t_len, seed0, with_actions, res, start_tries)
    else:
        drawn = draw_starts_device(preset, n_seq, t_len, seed0, with_actions, res, start_tries, dev)
    with np.errstate(divide='ignore', invalid='ignore'):          # (a sequence without a start runs from zero rows: 0 / 0)
        run = run_starts(drawn, t_len, device)
    out = {'X': run['X'], 'y': run['y'], 'in_bounds': run['in_bounds']}
    if drawn['actions'] is not None:
        rows = drawn['actions'].cpu().numpy() if isinstance(drawn['actions'], torch.Tensor) else drawn['actions']
        acts = np.zeros((n_seq, t_len, ACTIONS))
        for s in range(t_len):          # stored one step back, the wrap-around to the last row included (envs.py: acts[t - 1, a] = 1)
            acts[np.arange(n_seq), s - 1, rows[:, s]] = 1
        collisions = run['collisions']
        if isinstance(collisions, torch.Tensor):
            collisions = collisions.cpu().numpy()
        out['action'] = acts
        out['reward'] = -collisions.astype(np.float64)[:, :, None]
    return out, drawn.get('status')


# the reference's data-file generators (model/envs/envs.py: main, multi_billiards): run length 100, 1000 + 300 runs
DATA_NAMES = ('billiards', 'gravity', 'multibilliards', 'avoidance')
RUN_LEN, RUNS, MAX_TRIES = 100, (1000, 300), 10000


def _file_config(name, settings):
    """the config entries the reference writes beside the arrays, under its own argument names"""
    cfg = _envs.ENV_PRESETS[name]
    if name == 'avoidance':
        return {'res': settings['res'], 'hw': cfg['hw'], 'n': cfg['n'], 't': cfg['t'], 'm': cfg['m'], 'granularity': cfg['granularity'],
                'r': cfg['r'], 'friction_coefficient': cfg['friction_coefficient']}
    out = {'res': settings['res'], 'hw': cfg['hw'], 'n': cfg['n'], 'dt': cfg['t'], 'm': cfg['m'], 'fc': cfg['friction_coefficient'],
           'granularity': cfg['granularity'], 'r': cfg['r'], 'check_overlap': False}
    for k in ('init_v_factor', 'use_colors'):
        if k in cfg:
            out[k] = cfg[k]
    return out


def generate_runs(preset, run_num, t_len=RUN_LEN, seed0=0, res=None, device=None, chunk=256, max_tries=MAX_TRIES, filtered=True,
                  starts='host', start_tries=START_TRIES):
    """generate_fitting_run: candidates seed0, seed0 + 1, ... simulated in chunks, the first run_num accepted ones kept in seed order
    (filtered=False: every candidate is kept, as the reference keeps every avoidance run).  starts: as synth_sequences_batched; with
    'counter', a candidate without a start within start_tries attempts counts as rejected, filtered or not.
    -> (dict of host arrays as synth_sequences_batched returns, seeds kept (run_num,), number rejected)"""
    kept, seeds, bad, tried = [], [], 0, 0
    while len(seeds) < run_num and tried < max_tries:
        n = min(chunk, max_tries - tried)
        part, status = _synth_batched(preset, n, t_len, seed0 + tried, None, res, device, starts, start_tries)
        part = {k: (a.cpu().numpy() if isinstance(a, torch.Tensor) else a) for k, a in part.items()}
        good = accepted(part['in_bounds'], t_len, part['y'].shape[2]) if filtered else np.ones(n, dtype=bool)
        if status is not None:
            good = good & ((status.cpu().numpy() if isinstance(status, torch.Tensor) else status) == 0)
        idx = np.flatnonzero(good)[:run_num - len(seeds)]
        last = idx[-1] + 1 if len(seeds) + len(idx) >= run_num else n          # (candidates past the last one kept were never tried)
        bad += int((~good[:last]).sum())
        kept.append({k: a[idx] for k, a in part.items()})
        seeds.extend((seed0 + tried + idx).tolist())
        tried += n
    if len(seeds) < run_num:
        raise RuntimeError('only %d of %d runs were accepted within %d tries' % (len(seeds), run_num, max_tries))
    return {k: np.concatenate([p[k] for p in kept], 0) for k in kept[0]}, np.array(seeds), bad


def generate_data(name, out_dir='data', runs=RUNS, t_len=RUN_LEN, seed0=0, res=None, device=None, chunk=256, starts='host'):
    """The reference's `python -m model.envs.envs` for one of DATA_NAMES: <out_dir>/<name>_train.pkl and <name>_test.pkl with the keys
    the reference writes (X as (B, T, res, res, 3), y, the config entries, coord_lim; action, reward, done, action_space,
    action_force, type for avoidance).  The test file's candidates start where the train file's ended.  starts: 'host' or 'counter',
    as synth_sequences_batched.  -> the two paths"""
    if name not in DATA_NAMES:
        raise ValueError('generate_data writes %s, not %r' % (', '.join(DATA_NAMES), name))
    os.makedirs(out_dir, exist_ok=True)
    paths, seed = [], int(seed0)
    for kind, run_num in zip(('train', 'test'), runs):
        part, seeds, bad = generate_runs(name, int(run_num), t_len, seed, res, device, chunk, filtered=name != 'avoidance', starts=starts)
        print('Generation of {} runs finished, total amount of bad runs: {}. '.format(run_num, bad))
        seed = int(seeds[-1]) + 1 if len(seeds) else seed
        settings = draw_starts(name, 0, 1, res=res)['settings'] if starts == 'host' else _preset_settings(name, name == 'avoidance', res)[0]
        data = {'X': np.ascontiguousarray(np.transpose(part['X'], (0, 1, 3, 4, 2))).astype(np.float64), 'y': part['y']}
        if name == 'avoidance':
            data.update(action=part['action'], reward=part['reward'], done=np.zeros_like(part['reward']), type='AvoidanceTask',
                        action_force=settings['action_force'], action_space=ACTIONS)
        data.update(_file_config(name, settings))
        data['coord_lim'] = _envs.ENV_PRESETS[name]['hw']
        path = os.path.join(out_dir, '{}_{}.pkl'.format(name, kind))
        with open(path, 'wb') as f:
            pickle.dump(data, f, protocol=4)
        paths.append(path)
    return paths


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description='write <name>_train.pkl and <name>_test.pkl as the reference\'s model/envs/envs.py does')
    ap.add_argument('name', choices=DATA_NAMES)
    ap.add_argument('--out', default='data', help='directory of the two files')
    ap.add_argument('--device', default=None, help='a GPU (cuda:0): one launch per chunk of candidates; without it, numpy')
    ap.add_argument('--res', type=int, default=None, help='frame side (default: the preset\'s 32; the reference\'s stock gravity and '
                    'multibilliards files are 50)')
    ap.add_argument('--runs', type=int, nargs=2, default=list(RUNS), metavar=('TRAIN', 'TEST'))
    ap.add_argument('--seed0', type=int, default=0)
    ap.add_argument('--run-len', type=int, default=RUN_LEN)
    ap.add_argument('--chunk', type=int, default=256, help='candidates simulated together')
    ap.add_argument('--starts', choices=('host', 'counter'), default='host', help='host: the starts and actions of the reference\'s own '
                    'random stream, drawn in Python; counter: the counter-based stream (other numbers, the same distributions), drawn '
                    'on the GPU with --device')
    args = ap.parse_args(argv)
    if args.device is not None:
        from .. import build
        build.build_library()
    for p in generate_data(args.name, args.out, args.runs, args.run_len, args.seed0, args.res, args.device, args.chunk, args.starts):
        print(p)


if __name__ == '__main__':
    main()
