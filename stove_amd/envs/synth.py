"""Whole training sequences synthesised together: the batched counterpart of envs.synth_sequences and of the reference's data-file
command (model/envs/envs.py: generate_fitting_run, generate_data, generate_billiards_w_actions).

A step of an environment draws nothing, so all randomness of a sequence -- its start and, with actions, its action row -- is known
before it starts: `draw_starts` runs the constructors and the action policy exactly as envs.synth_sequences does and steps nothing.
`BatchedSequences` then simulates all B sequences together in numpy, vectorised over sequences with ELEMENTWISE ufuncs only, in the
operation order of stove_amd/csrc/env_step.h (billiards: BatchedAvoidance._step_rows / _draw) and stove_amd/csrc/env_gravity.h
(gravity: _gravity_rows, which restates PhysicsEnv.step + GravityEnv.simulate_physics with sqrt(a a + b b) norms and d * d * d cubes
where envs.py calls BLAS and pow).  On a GPU the same sequences are one ops.env_sequences call (stove_env_sequences,
csrc/env_sequences.hip), which reproduces the numpy states bit for bit; frames agree to one float32 ulp."""
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
    in_bounds, status then are device tensors) -> BatchedSequences.run's dict"""
    dev = _device(device)
    if dev is None:
        return BatchedSequences(starts).run(t_len, render=render)
    from .. import ops
    s = starts['settings']
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = ops.env_sequences(up(starts['x0']), up(starts['v0']), up(starts['r']), up(starts['m']), up(starts['actions']), t_len, s['granularity'],
                            s['res'], s['hw'], s['t'], s['friction'], s['action_force'], use_colors=s['use_colors'], drift=s['drift'],
                            gravity=s['gravity'], render=render)
    return dict(y=out['y'], X=out['frames'], collisions=out['collisions'], in_bounds=out['in_bounds'], status=out['status'])


def synth_sequences_batched(preset, n_seq, t_len, seed0=0, with_actions=None, res=None, device=None):
    """envs.synth_sequences with all sequences simulated together -> its dict (X (B,T,3,res,res) f32, y (B,T,n,4) f64 [, action (B,T,9),
    reward (B,T,1)]) plus in_bounds (B,).  device=None: the numpy specification, numpy arrays; a GPU device: one ops.env_sequences
    call, X, y and in_bounds device tensors (action and reward stay on the host: the actions were drawn there)."""
    starts = draw_starts(preset, n_seq, t_len, seed0, with_actions, res)
    run = run_starts(starts, t_len, device)
    out = {'X': run['X'], 'y': run['y'], 'in_bounds': run['in_bounds']}
    if starts['actions'] is not None:
        acts = np.zeros((n_seq, t_len, ACTIONS))
        for s in range(t_len):          # stored one step back, the wrap-around to the last row included (envs.py: acts[t - 1, a] = 1)
            acts[np.arange(n_seq), s - 1, starts['actions'][:, s]] = 1
        collisions = run['collisions']
        if isinstance(collisions, torch.Tensor):
            collisions = collisions.cpu().numpy()
        out['action'] = acts
        out['reward'] = -collisions.astype(np.float64)[:, :, None]
    return out


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


def generate_runs(preset, run_num, t_len=RUN_LEN, seed0=0, res=None, device=None, chunk=256, max_tries=MAX_TRIES, filtered=True):
    """generate_fitting_run: candidates seed0, seed0 + 1, ... simulated in chunks, the first run_num accepted ones kept in seed order
    (filtered=False: every candidate is kept, as the reference keeps every avoidance run).
    -> (dict of host arrays as synth_sequences_batched returns, seeds kept (run_num,), number rejected)"""
    kept, seeds, bad, tried = [], [], 0, 0
    while len(seeds) < run_num and tried < max_tries:
        n = min(chunk, max_tries - tried)
        part = synth_sequences_batched(preset, n, t_len, seed0 + tried, res=res, device=device)
        part = {k: (a.cpu().numpy() if isinstance(a, torch.Tensor) else a) for k, a in part.items()}
        good = accepted(part['in_bounds'], t_len, part['y'].shape[2]) if filtered else np.ones(n, dtype=bool)
        idx = np.flatnonzero(good)[:run_num - len(seeds)]
        last = idx[-1] + 1 if len(seeds) + len(idx) >= run_num else n          # (candidates past the last one kept were never tried)
        bad += int((~good[:last]).sum())
        kept.append({k: a[idx] for k, a in part.items()})
        seeds.extend((seed0 + tried + idx).tolist())
        tried += n
    if len(seeds) < run_num:
        raise RuntimeError('only %d of %d runs were accepted within %d tries' % (len(seeds), run_num, max_tries))
    return {k: np.concatenate([p[k] for p in kept], 0) for k in kept[0]}, np.array(seeds), bad


def generate_data(name, out_dir='data', runs=RUNS, t_len=RUN_LEN, seed0=0, res=None, device=None, chunk=256):
    """The reference's `python -m model.envs.envs` for one of DATA_NAMES: <out_dir>/<name>_train.pkl and <name>_test.pkl with the keys
    the reference writes (X as (B, T, res, res, 3), y, the config entries, coord_lim; action, reward, done, action_space,
    action_force, type for avoidance).  The test file's candidates start where the train file's ended.  -> the two paths"""
    if name not in DATA_NAMES:
        raise ValueError('generate_data writes %s, not %r' % (', '.join(DATA_NAMES), name))
    os.makedirs(out_dir, exist_ok=True)
    paths, seed = [], int(seed0)
    for kind, run_num in zip(('train', 'test'), runs):
        part, seeds, bad = generate_runs(name, int(run_num), t_len, seed, res, device, chunk, filtered=name != 'avoidance')
        print('Generation of {} runs finished, total amount of bad runs: {}. '.format(run_num, bad))
        seed = int(seeds[-1]) + 1 if len(seeds) else seed
        settings = draw_starts(name, 0, 1, res=res)['settings']
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
    args = ap.parse_args(argv)
    if args.device is not None:
        from .. import build
        build.build_library()
    for p in generate_data(args.name, args.out, args.runs, args.run_len, args.seed0, args.res, args.device, args.chunk):
        print(p)


if __name__ == '__main__':
    main()
