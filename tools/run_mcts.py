#!/usr/bin/env python
"""Play avoidance episodes with the tree search on a trained world model (reference scripts/run_mcts.py: main_mcts_model).

    python tools/run_mcts.py RUN_NAME CHECKPOINT_DIR [--envs 100 --mcts-steps 100 --depth 10 --run-len 100 --no-gifs]
                             [--device-envs] [--device-trees] [--fused-widths 16,32,64] [--policy random | env_mcts] [--replicas 1]

main_mcts_model restores the model (stove_amd.main.restore_model), builds the reference's environments -- BillardsEnv(n=3, hw=10,
r=1., res=32, seed=s) under AvoidanceTask(action_force=0.6), s = 0 .. envs - 1 -- and runs stove_amd.mcts.play.play on them:
as a list of host objects (the reference's loop; the default), or with --device-envs as one BatchedAvoidance stepped and rendered on
the model's device.  main_mcts_env (--policy env_mcts) is the reference's upper baseline: the search on the environments themselves
(stove_amd/mcts/mcts_env.py), no model.  The reference's own function refers to an `env` it never defines; here the environments,
the eight warm-up steps and the order of the returned rewards are main_mcts_model's (see main_mcts_env's docstring).  Returns (and
pickles to ./quicksave, as the reference does) the flat list of rewards in the order of the reference's main_mcts_model: step by step,
environment by environment.  GIFs of every environment go to ./RUN_NAME_0_<env>.gif."""
import argparse
import os
import pickle
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main_mcts_model(run_name, restore_point, save_gifs=True, num_parallel_envs=100, mcts_steps=100, max_rollout_depth=10, run_len=100,
                    device_envs=False, device_trees=False, policy='mcts', model=None, out_dir='.', replicas=1, fused_widths=None):
    """the reference's parameters, then the switches of this port (all off by default) -> the list of rewards"""
    from stove_amd.envs import envs
    from stove_amd.envs.batched import BatchedAvoidance
    from stove_amd.mcts.play import play
    from stove_amd.video_prediction.train import _save_clip
    if model is None and policy == 'mcts':
        from stove_amd.main import restore_model
        model = restore_model(restore_point)
    res = 32
    all_envs = [envs.AvoidanceTask(envs.BillardsEnv(n=3, hw=10, r=1., res=res, seed=s), 8, action_force=0.6) for s in range(num_parallel_envs)]
    if device_envs:
        dev = next(model.parameters()).device if model is not None else torch.device('cuda:0')
        all_envs = BatchedAvoidance.from_tasks(all_envs, device=dev)
    with torch.no_grad():
        out = play(model, all_envs, run_len=run_len, mcts_steps=mcts_steps, max_rollout_depth=max_rollout_depth, device_trees=device_trees,
                   policy=policy, keep_frames=save_gifs, replicas=replicas, fused_widths=fused_widths)
    results = [float(r) for r in out['rewards'].reshape(-1)]
    if save_gifs and run_len:
        clips = (255 * np.transpose(out['frames'], (1, 0, 2, 3, 4))).astype(np.uint8)            # (envs, run_len, 3, res, res)
        for i in range(num_parallel_envs):
            _save_clip(os.path.join(out_dir, '{}_{}_{}'.format(run_name, 0, i)), clips[i], fps=24)
    with open(os.path.join(out_dir, 'quicksave'), 'wb') as f:
        pickle.dump(results, f)
    return results


def main_mcts_env(run_name, save_gifs=True, num_parallel_envs=100, mcts_steps=100, max_rollout_depth=10, run_len=100, device_envs=False,
                  replicas=1, out_dir='.'):
    """the reference's parameters (it takes no restore point), then the switches of this port -> the list of rewards.  The reference's
    function steps an `env` it never defines, so it cannot be run as it stands; this one follows main_mcts_model in everything the
    reference leaves open or does differently: the environments are main_mcts_model's, every episode starts with its eight warm-up steps
    of action 0 (the reference's function has none), and the rewards come back step by step, environment by environment (the
    reference's appends them environment by environment, step by step: reshape (run_len, envs) and transpose for that order)."""
    return main_mcts_model(run_name, None, save_gifs=save_gifs, num_parallel_envs=num_parallel_envs, mcts_steps=mcts_steps,
                           max_rollout_depth=max_rollout_depth, run_len=run_len, device_envs=device_envs, policy='env_mcts',
                           out_dir=out_dir, replicas=replicas)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('run_name')
    ap.add_argument('restore_point', nargs='?', default=None, help='run directory of the trained action-conditioned model')
    ap.add_argument('--envs', type=int, default=100)
    ap.add_argument('--mcts-steps', type=int, default=100)
    ap.add_argument('--depth', type=int, default=10)
    ap.add_argument('--run-len', type=int, default=100)
    ap.add_argument('--no-gifs', action='store_true')
    ap.add_argument('--device-envs', action='store_true', help='step and render the environments on the device (off by default)')
    ap.add_argument('--device-trees', action='store_true', help='keep the search trees on the device (off by default)')
    ap.add_argument('--fused-widths', default=None, metavar='16,32,64', type=lambda v: tuple(int(w) for w in v.split(',')),
                    help='state-code lengths the fused expansion (and with it --device-trees) is offered at (default: 32 alone)')
    ap.add_argument('--policy', choices=('mcts', 'random', 'env_mcts'), default='mcts')
    ap.add_argument('--replicas', type=int, default=1, help='independent trees per environment with --policy env_mcts')
    ap.add_argument('--out-dir', default='.')
    args = ap.parse_args()
    if args.policy == 'mcts' and args.restore_point is None:
        ap.error('planning on a model needs a checkpoint: give restore_point (or --policy random / env_mcts)')
    results = main_mcts_model(args.run_name, args.restore_point, save_gifs=not args.no_gifs, num_parallel_envs=args.envs,
                              mcts_steps=args.mcts_steps, max_rollout_depth=args.depth, run_len=args.run_len, device_envs=args.device_envs,
                              device_trees=args.device_trees, policy=args.policy, out_dir=args.out_dir, replicas=args.replicas,
                              fused_widths=args.fused_widths)
    print('mean reward per step %.4f (std %.4f) over %d environment steps' % (np.mean(results), np.std(results), len(results)))


if __name__ == '__main__':
    main()
