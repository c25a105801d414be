"""Shared sequences of the data-synthesis tests (tests/test_env_sequences_cpu.py, tests/test_gpu_env_sequences.py): the cases, their
starts (draw_starts), the numpy specification's run (computed once per case, never modified) and an instrumented envs.py side."""
import functools

import numpy as np

from stove_amd.envs import envs, synth
from env_cases import Recording

_B3 = dict(envs.ENV_PRESETS['billiards'])
_G3 = dict(envs.ENV_PRESETS['gravity'])
# name -> (preset name or config, T, with actions, res or None, seeds)
CASES = {
    'bill3': ('billiards', 12, False, None, (1, 2, 3, 5)),
    'bill6': ('multibilliards', 12, False, None, (0, 2, 3, 4)),
    'avoid3': ('avoidance', 12, True, None, (2, 7, 9, 10)),
    'bill1': (dict(_B3, n=1), 12, False, None, (0, 1, 2, 3)),
    'drift3': (dict(_B3, drift=True), 12, False, None, (1, 2, 5, 6)),
    'fric3': (dict(_B3, friction_coefficient=0.05), 12, False, None, (2, 3, 5, 6)),
    'grav3': ('gravity', 12, False, None, (0, 1, 2, 3)),
    'grav2': (dict(_G3, n=2), 12, False, None, (0, 1, 2, 3)),
    'grav_clip': (dict(_G3, m=12.), 12, False, None, (0, 3, 4, 5)),
    'grav_out': (dict(_G3, init_v_factor=1.2), 12, False, None, (4, 5, 6, 7)),
    'bill3_T1': ('billiards', 1, False, None, (1, 2, 3, 5)),
    'bill3_T2': ('billiards', 2, False, None, (1, 2, 3, 5)),
    'bill3_T3': ('billiards', 3, False, None, (1, 2, 3, 5)),
    'grav3_T1': ('gravity', 1, False, None, (0, 1, 2, 3)),
    'grav3_T2': ('gravity', 2, False, None, (0, 1, 2, 3)),
    'grav3_T3': ('gravity', 3, False, None, (0, 1, 2, 3)),
    'res8': ('billiards', 12, False, 8, (1, 2, 3, 5)),
    'res50': ('gravity', 12, False, 50, (0, 1, 2, 3)),
}
# The seeds were searched on the CPU among 0 .. 39, one envs.py run (instrumented, envs_run) per seed: kept are seeds whose every branch
# margin over the run -- |next - r|, |next - (hw - r)| per ball and axis, |gap - (r_i + r_j)| per pair, | |f| - 1 | per force component,
# and the distance of every recorded coordinate from 0 and hw -- is an exact tie that any arithmetic reproduces or >= 1e-4 (the tests
# ask for 1e-6 and exclude nothing), preferring seeds with wall bounces and collisions: avoidance seeds 2, 7, 9, 10 have 1, 3, 11 and 10
# controlled collisions; billiards seeds 1, 2, 3, 5 have 4, 1, 1, 2 wall bounces and 0, 1, 1, 2 free collisions.  grav_clip: with m = 12
# the pair force 72 / d^2 exceeds 1 below d = 8.5 -- seeds 0, 4, 5 clip 1222, 1888 and 891 components over the run, seed 3 none.
# grav_out: init_v_factor 1.2 (0.8 kept all of seeds 0 .. 15, 1.0 rejected two, 1.5 rejected all); seeds 4, 5, 6, 7 are consecutive and are
# accepted, rejected (71 of 72 coordinates inside), accepted, rejected, so the first two accepted runs from seed 4 on are seeds 4 and 6.


class RecordingGravity(envs.GravityEnv):
    """GravityEnv.simulate_physics, statement for statement, with the margin of the force clip written down: | |f| - 1 | of every
    component before the clip, and how many components the clip changed."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.margins, self.clipped = [], 0

    def simulate_physics(self, actions):
        mid = np.array([self.hw / 2, self.hw / 2])
        v = np.zeros_like(self.v)
        for i in range(self.n):
            force = np.array([0., 0.])
            for j in range(self.n):
                if i != j:
                    dist = np.linalg.norm(self.x[j] - self.x[i])
                    force -= self.G * self.m[j] * self.m[i] * (self.x[i] - self.x[j]) / ((dist + 1e-5) ** 3)
            to_mid = mid - self.x[i]
            force += 0.001 * (to_mid ** 3) / envs._row_norm(to_mid)
            self.margins.extend((abs(abs(float(f)) - 1.0), False) for f in force)
            self.clipped += int((np.abs(force) > 1).sum())
            force = np.clip(force, -1, 1)
            v[i] = self.v[i] + (force / self.m[i]) * self.t * self.eps
        return v


def _seed_env(name, seed, recording):
    preset, _, _, res, _ = CASES[name]
    cfg = synth._config(preset)
    if res is not None:
        cfg['res'] = res
    kind = cfg.pop('cls')
    cls = {('billiards', False): envs.BillardsEnv, ('gravity', False): envs.GravityEnv, ('billiards', True): Recording,
           ('gravity', True): RecordingGravity}[kind, recording]
    return cls(seed=seed, **cfg)


@functools.lru_cache(maxsize=None)
def starts(name):
    """draw_starts of case `name` (seeds need not be consecutive: one call per seed, stacked), shared and read only"""
    preset, T, acting, res, seeds = CASES[name]
    parts = [synth.draw_starts(preset, 1, T, seed0=s, with_actions=acting, res=res) for s in seeds]
    out = {k: (np.concatenate([p[k] for p in parts], 0) if parts[0][k] is not None else None) for k in ('x0', 'v0', 'r', 'm', 'actions')}
    out['settings'] = parts[0]['settings']
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def host_run(name):
    """the numpy specification's run of case `name` -> BatchedSequences.run's dict, read only"""
    out = synth.BatchedSequences(starts(name)).run(CASES[name][1])
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def envs_run(name, recording=True):
    """the same sequences on envs.py, in synth_sequences' loop (recording: on the instrumented classes) -> dict(X, y [, action,
    reward], in_bounds; margins [(margin, tie)] of every branch -- walls, pair gaps, the force clip, and the box bounds of every
    recorded coordinate --, clip_margins and bound_margins: the last two kinds alone, clipped: components the force clip changed, envs: the environments)"""
    _, T, acting, _, seeds = CASES[name]
    X, Y, A, R, margins, bounds, all_envs, counts = [], [], [], [], [], [], [], []
    for seed in seeds:
        env = _seed_env(name, seed, recording)
        imgs, states = [], []
        if acting:
            task = envs.AvoidanceTask(env, 4, greyscale=False, action_force=0.6)
            policy = envs.MonteCarloActionPolicy(9, env.rng.uniform(0.2, 0.3), rng=env.rng)
            acts, rews = np.zeros((T, 9)), np.zeros((T, 1))
        for t in range(T):
            if acting:
                a = policy.next()
                img, st, rew, _ = task.step(a)
                acts[t - 1, a] = 1
                rews[t] = rew
            else:
                img, st, _ = env.step()
            imgs.append(img)
            states.append(st)
        if acting:
            A.append(acts)
            R.append(rews)
        X.append(np.stack(imgs))
        Y.append(np.stack(states))
        pos = Y[-1][:, :, :2]
        bounds.extend(float(d) for d in np.minimum(np.abs(pos), np.abs(pos - env.hw)).ravel())
        counts.append(int(((pos > 0) & (pos < env.hw)).sum()))
        margins.extend(getattr(env, 'margins', []))
        all_envs.append(env)
    out = {'X': np.transpose(np.stack(X), (0, 1, 4, 2, 3)).astype(np.float32), 'y': np.stack(Y), 'in_bounds': np.array(counts),
           'margins': margins + [(d, False) for d in bounds], 'bound_margins': bounds,
           'clip_margins': [d for e in all_envs if isinstance(e, RecordingGravity) for d, _ in e.margins], 'clipped': sum(getattr(e, 'clipped', 0) for e in all_envs), 'envs': all_envs}
    if acting:
        out['action'], out['reward'] = np.stack(A), np.stack(R)
    return out
