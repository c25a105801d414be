"""Shared cases of the tests of the PPO arm's collection (tests/test_ppo_cpu.py, tests/test_gpu_ppo.py): the reference's recorded policy
outputs (tests/golden/g24_ppo.npz, tools/make_ppo_goldens.py), the seeded shape cases, and the host forest's collection of each
(computed once per case, never modified)."""
import functools
import json
import os

import numpy as np
import torch

from stove_amd.envs.batched import BatchedAvoidance
from stove_amd.rl.collect import KEYS, PolicyForest
from stove_amd.rl.rl_model import Policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, WARMUP, DISCOUNT, MIN_MARGIN = 9, 1, 0.95, 1e-9
# name -> (B, S, N, H, deep, granularity, friction, drift, environment seeds).  Environment b starts from BatchedAvoidance(seed) after one
# step with action 0 (as the runner starts a trajectory) and reads the uniforms of RandomState(900 + seed), so a trajectory does not
# depend on its batch.  The seeds are those, in order from 0, whose smallest decision margin in the host forest over the whole
# trajectory is >= 1e-9 (asserted by the tests, no environment left out): with float32 uniforms a draw violates that with a chance of
# about 2e-8, so no seed had to be passed over.
CASES = {
    'b1_s1_n1_h32': (1, 1, 1, 32, False, 5, 0.0, False, (0,)),
    'b3_s5_n3_h64': (3, 5, 3, 64, False, 5, 0.0, False, (0, 1, 2)),
    'b5_s16_n6_h64_deep': (5, 16, 6, 64, True, 5, 0.0, False, (0, 1, 2, 3, 4)),          # more environments than a block; the widest obs
    'b4_s8_n3_h40': (4, 8, 3, 40, False, 5, 0.0, False, (0, 1, 2, 3)),                   # H no multiple of the wave or of 32
    'b4_s8_n3_h128_deep': (4, 8, 3, 128, True, 5, 0.0, False, (0, 1, 2, 3)),             # the image that does not fit LDS
    'b4_s8_n3_g2': (4, 8, 3, 64, False, 2, 0.0, False, (0, 1, 2, 3)),                    # main_rl's defaults: granularity 2, force .3
    'b4_s8_n3_fric': (4, 8, 3, 64, False, 5, 0.05, False, (0, 1, 2, 3)),
    'b32_s128_n3_h64': (32, 128, 3, 64, False, 5, 0.0, False, tuple(range(32))),         # the workload, once
}
ACTION_FORCE = {'b4_s8_n3_g2': 0.3}          # every other case: AvoidanceTask's 0.6 of the planning experiments
for _name, _c in CASES.items():
    assert _c[0] == len(_c[8]), _name


def action_force(name):
    return ACTION_FORCE.get(name, 0.6)


@functools.lru_cache(maxsize=None)
def policy(N, H, deep):
    """Policy(base='control') with seeded weights: every tensor uniform in +-1 / sqrt(fan_in) from numpy, the actor head six times as
    large and its bias in +-1, so that the nine probabilities are visibly unequal and the draw matters.  Shared: never trained."""
    p = Policy(4 * N, A, hidden_size=H, base='control', use_deep_layers=deep)
    rs = np.random.RandomState(7000 + 100 * N + H + (50 if deep else 0))
    state, sd = {}, p.state_dict()
    for key, ten in sd.items():
        weight = sd[key[:-len('bias')] + 'weight'] if key.endswith('bias') else ten
        bound = {'head.actor_head.weight': 6.0, 'head.actor_head.bias': float(np.sqrt(weight.shape[1]))}.get(key, 1.0) / np.sqrt(weight.shape[1])
        state[key] = torch.from_numpy(rs.uniform(-bound, bound, size=tuple(ten.shape)).astype(np.float32))
    p.load_state_dict(state)
    for q in p.parameters():
        q.requires_grad_(False)
    return p


def envs(name, device=None):
    """a fresh BatchedAvoidance at the case's start state (the caller may step it)"""
    B, S, N, H, deep, gran, fric, drift, seeds = CASES[name]
    b = BatchedAvoidance(seeds, n=N, granularity=gran, action_force=action_force(name), friction_coefficient=fric, drift=drift)
    for _ in range(WARMUP):
        b.step(np.zeros(b.M, dtype=np.int64), render=False)
    return b.to(device) if device is not None else b


@functools.lru_cache(maxsize=None)
def table(name):
    """u (B, S) float32 in [0, 1); read only"""
    S, seeds = CASES[name][1], CASES[name][8]
    u = np.stack([np.random.RandomState(900 + s).random_sample(S) for s in seeds]).astype(np.float32).reshape(len(seeds), S)
    u = np.minimum(u, np.float32(1) - np.float32(2) ** -24)
    u.setflags(write=False)
    return u


@functools.lru_cache(maxsize=None)
def host_collect(name):
    """-> (the collection dict of the host forest, final x, final v, margin (B,)); read only"""
    B, S, N, H, deep = CASES[name][:5]
    f = PolicyForest.from_policy(policy(N, H, deep))
    b = envs(name)
    out = f.collect(b, table(name), DISCOUNT)
    for a in list(out.values()) + [b.x, b.v, f.margin]:
        a.setflags(write=False)
    assert set(out) == set(KEYS)
    return out, b.x, b.v, f.margin


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'g24_ppo.npz'))


@functools.lru_cache(maxsize=None)
def fp32_gap():
    with open(os.path.join(ROOT, 'tests', 'golden', 'g24_reference_fp32_gap.json')) as fh:
        return json.load(fh)


GOLDEN_SHAPES = ((3, 64, False), (6, 64, True), (1, 32, False))


def golden_policy(case, dtype=torch.float32):
    """the reference's seeded Policy of golden case `case`, rebuilt on this project's classes from its recorded state_dict"""
    N, H, deep = GOLDEN_SHAPES[case]
    G = golden()
    p = Policy(4 * N, A, hidden_size=H, base='control', use_deep_layers=deep)
    pre = 'c%d_sd_' % case
    p.load_state_dict({k[len(pre):]: torch.from_numpy(G[k]) for k in G.files if k.startswith(pre)})
    return p.to(dtype)


def ulps32(a, b):
    """the distance of two float32 arrays in units in the last place (same-sign finite values)"""
    ia, ib = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64), np.ascontiguousarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)
