"""Shared cases of the tests of the PPO arm's collection on images (tests/test_ppo_image_cpu.py, tests/test_gpu_ppo_image.py): the
reference's recorded frame buffers and policy outputs (tests/golden/g26_ppo_images.npz, tools/make_ppo_image_goldens.py), the seeded
shape cases, the host forest's collection of each (computed once per case, never modified) and the compositional comparison both the
CPU driver and the kernel are held to."""
import functools
import json
import os

import numpy as np
import torch

from stove_amd.envs.batched import BatchedAvoidance
from stove_amd.rl.collect import IMAGE_KEYS, ImageForest
from stove_amd.rl.rl_model import Policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, DISCOUNT, MIN_MARGIN, ACTION_FORCE = 9, 0.95, 1e-6, 0.3
# name -> (B, S, N, F, H, deep, warm, granularity).  Environment b is BatchedAvoidance(seed b) as constructed (the warm-up belongs to the
# collection) and reads the uniforms of RandomState(2600 + b): a trajectory does not depend on its batch.
CASES = {
    'b5_s3_n3_f4_h16': (5, 3, 3, 4, 16, False, 4, 2),
    'b2_s2_n6_f4_h512_deep': (2, 2, 6, 4, 512, True, 4, 2),          # the widest head, every layer
    'b3_s4_n1_f1_h1': (3, 4, 1, 1, 1, False, 1, 5),                  # one object, one frame, one neuron, the shortest warm-up
    'b9_s2_n2_f2_h33_deep': (9, 2, 2, 2, 33, True, 4, 2),            # a head that ends inside a wave, a warm-up longer than the window
    'b4_s3_n3_f3_h64': (4, 3, 3, 3, 64, False, 2, 2),                # a window longer than the warm-up: zero rows
}


@functools.lru_cache(maxsize=None)
def policy(F, H, deep):
    """Policy((32, 32, 3F), 9) with seeded weights: every tensor uniform in +-1 / sqrt(fan_in) from numpy; the first convolution 255
    times as large, which undoes the division of frames that are already in [0, 1], so that the frames matter; the actor head six times
    as large and its bias in +-1, so that the nine probabilities are visibly unequal and the draw matters.  Shared: never trained."""
    p = Policy((32, 32, 3 * F), A, hidden_size=H, stacked_frames=F, use_deep_layers=deep)
    rs = np.random.RandomState(26000 + 1000 * F + H + (700 if deep else 0))
    state, sd = {}, p.state_dict()
    for key, ten in sd.items():
        weight = sd[key[:-len('bias')] + 'weight'] if key.endswith('bias') else ten
        fan_in = weight[0].numel()
        bound = {'base.main.0.weight': 255.0, 'head.actor_head.weight': 6.0, 'head.actor_head.bias': float(np.sqrt(fan_in))}.get(key, 1.0) / np.sqrt(fan_in)
        state[key] = torch.from_numpy(rs.uniform(-bound, bound, size=tuple(ten.shape)).astype(np.float32))
    p.load_state_dict(state)
    for q in p.parameters():
        q.requires_grad_(False)
    return p


def envs(name, device=None):
    """a fresh BatchedAvoidance at the case's start state (the caller may step it)"""
    B, S, N, F, H, deep, warm, gran = CASES[name]
    b = BatchedAvoidance(range(B), n=N, granularity=gran, action_force=ACTION_FORCE)
    return b.to(device) if device is not None else b


@functools.lru_cache(maxsize=None)
def table(name):
    """u (B, S) float32 in [0, 1); read only"""
    B, S = CASES[name][:2]
    u = np.stack([np.random.RandomState(2600 + b).random_sample(S) for b in range(B)]).astype(np.float32).reshape(B, S)
    u = np.minimum(u, np.float32(1) - np.float32(2) ** -24)
    u.setflags(write=False)
    return u


@functools.lru_cache(maxsize=None)
def forest(F, H, deep):
    return ImageForest.from_policy(policy(F, H, deep))


@functools.lru_cache(maxsize=None)
def host_collect(name):
    """-> (the collection dict of the host forest, final x, final v, margin (B,)); read only"""
    B, S, N, F, H, deep, warm, gran = CASES[name]
    f = forest(F, H, deep)
    b = envs(name)
    out = f.collect(b, table(name), DISCOUNT, warm)
    margin = f.margin.copy()
    for a in list(out.values()) + [b.x, b.v, margin]:
        a.setflags(write=False)
    assert set(out) == set(IMAGE_KEYS)
    return out, b.x, b.v, margin


def ulps32(a, b):
    """the distance of two float32 arrays in units in the last place (same-sign finite values)"""
    ia, ib = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64), np.ascontiguousarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def assert_composes(got, name):
    """`got`: what the CPU driver or the kernel collected on case `name` -- frames, actions, rewards, values, logp, next_value, returns,
    status and the final x, v as numpy arrays.  Compositionally against the specification:
      handed these very frames, ImageForest.decide returns the same values, next_value and actions bit for bit and logp to one float32
      ulp, every draw with a margin >= MIN_MARGIN (no draw is left out);
      the host BatchedAvoidance under `warm` steps with action 0 and then these actions has the same x, v and rewards bit for bit, and
      its frames equal these to one float32 ulp (exp is a library call on either side; the zero rows are zero);
      returns equal Runner._calculate_returns on these rewards and next_value bit for bit.
    -> (the largest logp distance in ulp, the largest frame distance in ulp, the smallest margin)"""
    from stove_amd.rl.runners import Runner
    B, S, N, F, H, deep, warm, gran = CASES[name]
    bits = lambda a: np.ascontiguousarray(a).view(np.int32 if a.dtype.itemsize == 4 else np.int64)
    assert got['status'].tolist() == [0] * B
    frames = got['frames']
    assert frames.shape == (B, F + S, 3, 32, 32) and frames.dtype == np.float32
    # ---- the policy half
    f = forest(F, H, deep)
    windows = np.stack([frames[:, s:s + F] for s in range(S + 1)], axis=1).reshape(B * (S + 1), F, 3, 32, 32)
    u = np.concatenate([table(name), np.zeros((B, 1), np.float32)], axis=1).reshape(-1)
    values, actions, logp, margin = f.decide(windows, u)
    values, actions, logp, margin = (a.reshape(B, S + 1) for a in (values, actions, logp, margin))
    assert (margin[:, :S] >= MIN_MARGIN).all(), margin[:, :S].min()
    assert np.array_equal(bits(got['values']), bits(values[:, :S])) and np.array_equal(bits(got['next_value']), bits(values[:, S]))
    assert np.array_equal(got['actions'], actions[:, :S])
    worst_logp = int(ulps32(got['logp'], logp[:, :S]).max()) if S else 0
    assert worst_logp <= 1, worst_logp
    # ---- the environment half
    b = envs(name)
    rows = np.zeros((B, F + S, 3, 32, 32), np.float32)
    for w in range(warm):
        img, _ = b.step(np.zeros(B, dtype=np.int64))
        if F - warm + w >= 0:
            rows[:, F - warm + w] = img
    rewards = np.zeros((B, S), np.float32)
    for s in range(S):
        rows[:, F + s], reward = b.step(got['actions'][:, s])
        rewards[:, s] = reward
    assert np.array_equal(bits(got['x']), bits(b.x)) and np.array_equal(bits(got['v']), bits(b.v))
    assert np.array_equal(bits(got['rewards']), bits(rewards))
    assert not frames[:, :max(F - warm, 0)].any() and (frames >= 0).all() and rows[:, F - min(warm, F):].any(axis=(2, 3, 4)).all()
    worst_frame = int(ulps32(frames, rows).max())
    assert worst_frame <= 1, worst_frame
    # ---- the returns
    runner = Runner.__new__(Runner)
    runner.discount = DISCOUNT
    three = lambda a: torch.from_numpy(np.array(a)).reshape(B, S, 1)
    want = runner._calculate_returns(torch.from_numpy(np.array(got['next_value'])).reshape(B, 1), three(got['rewards']),
                                     torch.zeros(B, S, 1)).numpy()[:, :, 0]
    assert want.dtype == np.float32 and np.array_equal(bits(got['returns']), bits(want))
    return worst_logp, worst_frame, float(margin[:, :S].min()) if S else float('inf')


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'g26_ppo_images.npz'))


@functools.lru_cache(maxsize=None)
def fp32_gap():
    with open(os.path.join(ROOT, 'tests', 'golden', 'g26_reference_fp32_gap.json')) as fh:
        return json.load(fh)


GOLDEN_SHAPES = ((4, 16, False), (2, 8, True))


def golden_task(case):
    """this package's environment and task with the settings the fixture's were recorded under"""
    from stove_amd.envs import envs as E
    F = GOLDEN_SHAPES[case][0]
    return E.AvoidanceTask(E.BillardsEnv(n=3, granularity=2, seed=60 + case), num_stacked=F, action_force=.3)


def golden_policy(case, dtype=torch.float32):
    """the reference's seeded image policy of golden case `case`, rebuilt on this project's classes from its recorded state_dict"""
    F, H, deep = GOLDEN_SHAPES[case]
    G = golden()
    p = Policy((32, 32, 3 * F), A, hidden_size=H, stacked_frames=F, use_deep_layers=deep)
    pre = 'c%d_sd_' % case
    p.load_state_dict({k[len(pre):]: torch.from_numpy(G[k]) for k in G.files if k.startswith(pre)})
    return p.to(dtype)


def golden_windows(case):
    """the fixture's four frame buffers (4, 32, 32, 3F) float64 as float32 windows (4, F, 3, 32, 32), oldest frame first"""
    F = GOLDEN_SHAPES[case][0]
    buf = golden()['c%d_buf' % case]
    return np.ascontiguousarray(buf.transpose(0, 3, 1, 2).reshape(4, F, 3, 32, 32).astype(np.float32))
