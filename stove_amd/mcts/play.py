"""Closed-loop planning: play avoidance episodes with the tree search on the learned model (reference scripts/run_mcts.py:
main_mcts_model; policy='random' is scripts/random_env_baseline.py; policy='env_mcts' is main_mcts_env, the search on the
environments themselves, mcts_env.py).

Eight warm-up steps with action 0 fill a ring of the last 8 frames and a ring of the last 8 one-hot actions; then per step: plan on
the rings, step every environment with the chosen action, shift both rings.  On a list of AvoidanceTask this is the reference's loop on
initialize_img / run_mcts_model's planner / update_buffer, unchanged.  On a BatchedAvoidance the rings (M, 8, 3, res, res) float32 and
(M, 8, 9) live where the environments live (numpy on the host, tensors on the device) and the planner takes the frames as they are
(plan_on_frames): with device environments no frame crosses the host."""
import numpy as np
import torch

from ..envs.batched import ACTIONS, BatchedAvoidance
from .mcts_env import plan_on_envs
from .mcts_stove import initialize_img, plan_on_frames, plan_on_model, update_buffer

WARMUP = 8


class Rings:
    """the last WARMUP frames (M, 8, 3, res, res) float32 and one-hot actions (M, 8, 9) float32 of a BatchedAvoidance, oldest first"""

    def __init__(self, envs):
        self.envs = envs
        lib = np if envs.device is None else torch
        kw = {} if envs.device is None else {'device': envs.device}
        self.frames = lib.zeros((envs.M, WARMUP, 3, envs.res, envs.res), dtype=lib.float32, **kw)
        self.actions = lib.zeros((envs.M, WARMUP, ACTIONS), dtype=lib.float32, **kw)

    def push(self, frames, actions):
        """shift both rings by one and append `frames` (M, 3, res, res) and the one-hot rows of `actions` (M,) ints"""
        if self.envs.device is None:
            self.frames[:, :-1] = self.frames[:, 1:]
            self.actions[:, :-1] = self.actions[:, 1:]
        else:
            self.frames[:, :-1] = self.frames[:, 1:].clone()
            self.actions[:, :-1] = self.actions[:, 1:].clone()
        self.frames[:, -1] = frames
        self.actions[:, -1] = 0
        a = np.asarray(actions).astype(np.int64).reshape(-1)
        rows = np.arange(self.envs.M)
        if self.envs.device is None:
            self.actions[rows, -1, a] = 1
        else:
            self.actions[torch.from_numpy(rows).to(self.envs.device), -1, torch.from_numpy(a).to(self.envs.device)] = 1

    def step(self, actions):
        """step the environments with `actions` (M,) and push the result -> (reward (M,) numpy, state (M, N, 4) numpy)"""
        frames, reward = self.envs.step(actions)
        status = self.envs.status if self.envs.device is None else self.envs.status.cpu().numpy()
        if status.any():
            raise RuntimeError('environment %d refused its action index %r' % (int(np.flatnonzero(status)[0]), actions))
        self.push(frames, actions)
        state = self.envs.state()
        if self.envs.device is not None:
            reward, state = reward.cpu().numpy(), state.cpu().numpy()
        return np.asarray(reward), np.asarray(state)

    def tensors(self):
        """(frames, actions) as the planner takes them"""
        if self.envs.device is None:
            return torch.from_numpy(self.frames), torch.from_numpy(self.actions)
        return self.frames, self.actions


def warm_up(envs):
    """WARMUP steps with action 0 -> the filled Rings of a BatchedAvoidance"""
    rings = Rings(envs)
    for _ in range(WARMUP):
        rings.step(np.zeros(envs.M, dtype=np.int64))
    return rings


def play(model, envs, run_len=100, mcts_steps=100, max_rollout_depth=10, fused=None, device_trees=False, policy='mcts', keep_frames=False,
         replicas=1, fused_widths=None):
    """One episode of every environment.  envs: a BatchedAvoidance (host or device) or a list of AvoidanceTask (the reference's
    per-environment loop).  policy: 'mcts' plans with `mcts_steps` expansions per tree on `model` (an action-conditioned Stove);
    'random' draws one np.random.randint(9, size=M) per step and needs no model; 'env_mcts' searches the environments themselves
    (mcts_env.plan_on_envs: `replicas` trees of `mcts_steps` iterations per environment, one np.random.randint(9, size=(M replicas,
    mcts_steps, max_rollout_depth)) per step), needs no model either and looks at no frame; a list of AvoidanceTask goes through
    BatchedAvoidance.from_tasks for the search only.  fused_widths: the state-code lengths the fused expansion is offered at (None:
    mcts_stove.FUSED_WIDTHS), as plan_on_frames takes it.  It raises ValueError for max_rollout_depth < 2, whatever run_len is.
    -> dict(actions (run_len, M) int64, rewards (run_len, M) float64, states (run_len, M, N, 4) float64 [, frames (run_len, M, 3, res,
    res) float32 with keep_frames]), the warm-up steps not included."""
    if policy not in ('mcts', 'random', 'env_mcts'):
        raise ValueError("policy is 'mcts', 'random' or 'env_mcts', not %r" % (policy,))
    if policy == 'env_mcts' and max_rollout_depth < 2:
        raise ValueError('the search on the environments needs max_rollout_depth >= 2, not %r' % (max_rollout_depth,))
    if policy == 'mcts' and model is None:
        raise ValueError("policy='mcts' plans on a model")
    batched = isinstance(envs, BatchedAvoidance)
    M = envs.M if batched else len(envs)
    if batched:
        rings = warm_up(envs)
    else:
        img, actions = initialize_img(envs, steps=WARMUP, res=envs[0].env.res)
    out = {'actions': [], 'rewards': [], 'states': [], 'frames': []}
    for _ in range(run_len):
        if policy == 'random':
            nxt = [int(a) for a in np.random.randint(ACTIONS, size=M)]
        elif policy == 'env_mcts':
            nxt = plan_on_envs(envs if batched else BatchedAvoidance.from_tasks(envs), mcts_steps, max_rollout_depth, replicas)
        elif batched:
            x, acts = rings.tensors()
            nxt = plan_on_frames(x, model, acts, M, mcts_steps, max_rollout_depth, fused, device_trees, fused_widths)
        else:
            nxt = plan_on_model(img, model, actions, M, mcts_steps, max_rollout_depth, fused, device_trees, fused_widths)
        if batched:
            reward, state = rings.step(nxt)
            frame = rings.frames[:, -1]
            if keep_frames:
                out['frames'].append(np.array(frame) if envs.device is None else frame.cpu().numpy())
        else:
            new_img, state, reward = np.zeros((M,) + img.shape[2:]), [], []
            for j in range(M):
                new_img[j], st, r, _ = envs[j].step(nxt[j])
                state.append(st)
                reward.append(r)
            img, actions = update_buffer(img, new_img, actions, nxt)
            if keep_frames:
                out['frames'].append(np.transpose(new_img, (0, 3, 1, 2)).astype(np.float32))
        out['actions'].append(np.asarray(nxt, dtype=np.int64))
        out['rewards'].append(np.asarray(reward, dtype=np.float64))
        out['states'].append(np.asarray(state, dtype=np.float64))
    n_obj = envs.n if batched else envs[0].env.n
    res = {'actions': np.stack(out['actions']) if run_len else np.zeros((0, M), dtype=np.int64),
           'rewards': np.stack(out['rewards']) if run_len else np.zeros((0, M)),
           'states': np.stack(out['states']) if run_len else np.zeros((0, M, n_obj, 4))}
    if keep_frames:
        res['frames'] = np.stack(out['frames']) if run_len else np.zeros((0, M, 3, 0, 0), dtype=np.float32)
    return res
