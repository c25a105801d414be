#!/usr/bin/env python
"""Time one planning step of the search on the true environment (stove_amd/mcts/mcts_env.py) at the reference's shape: 100 avoidance
environments (n = 3, hw = 10, r = 1, granularity 5), 100 expansions per tree, rollout depth 10, with R = 1 and R = 32 trees per
environment.

    python tools/env_search_time.py [--envs 100 --steps 100 --depth 10 --replicas 1 32 --repeats 5 --object-envs 10
                                     --out profiles/env_search.json]

Per planning step of the whole batch, in ms:
  object_loop  MCTS(task, depth).run_mcts(steps) environment by environment (what the reference's main_mcts_env does).  Timed on the
               first --object-envs environments and scaled to --envs (the trees are independent; both figures are written down), and at
               R = 1 only: R trees are R times the work by construction.
  numpy        EnvForest.search on the host BatchedAvoidance: numpy over all trees in lock step
  device       one ops.env_search on the device BatchedAvoidance (table and fresh arrays already there), ended by a device synchronise
The paths run in one process after a warm-up of each, in an order that rotates from repeat to repeat; median and range of the repeats
are reported.  Also recorded: the summed return of one short episode batch (--episode-len steps of every environment) under
policy='env_mcts' on the device and under policy='random'.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=100)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--depth', type=int, default=10)
    ap.add_argument('--replicas', type=int, nargs='+', default=[1, 32])
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--object-envs', type=int, default=10)
    ap.add_argument('--episode-len', type=int, default=30)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'env_search.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('env_search_time.py measures on a GPU; none found')
    from stove_amd import ops
    from stove_amd.envs import envs
    from stove_amd.envs.batched import ACTIONS, BatchedAvoidance
    from stove_amd.mcts.mcts_env import MCTS, EnvForest
    from stove_amd.mcts.play import play
    dev = torch.device('cuda:0')
    M, runs, D = args.envs, args.steps, args.depth
    K = min(args.object_envs, M)
    make = lambda: [envs.AvoidanceTask(envs.BillardsEnv(n=3, hw=10, r=1., res=32, seed=s), action_force=0.6) for s in range(M)]
    tasks = make()
    host = BatchedAvoidance.from_tasks(tasks)
    device = BatchedAvoidance.from_tasks(tasks, device=dev)
    rs = np.random.RandomState(0)

    def object_loop(steps=runs):
        np.random.seed(int(rs.randint(1 << 30)))
        t0 = time.perf_counter()
        for j in range(K):
            MCTS(tasks[j], max_rollout=D).run_mcts(steps)
        return (time.perf_counter() - t0) * M / K

    def numpy_search(R, steps=runs):
        draws = rs.randint(ACTIONS, size=(M * R, steps, D))
        t0 = time.perf_counter()
        EnvForest(M * R, ACTIONS, D, steps).search(host, draws, R)
        return time.perf_counter() - t0

    def device_search(R, steps=runs):
        draws = torch.from_numpy(rs.randint(ACTIONS, size=(M * R, steps, D)).astype(np.int32)).to(dev)
        arrays = EnvForest(M * R, ACTIONS, D, steps).to_device(dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ops.env_search(device.x, device.v, device.r, device.m, draws, arrays, D, device.granularity, device.hw, device.t, device.friction,
                       device.action_force, device.drift, replicas=R)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if int(arrays['status'].abs().sum()):
            raise RuntimeError('a tree of the timed search ended with a non-zero status')
        return dt

    pieces = [('object_loop', object_loop)]
    for R in args.replicas:
        pieces += [('numpy_R%d' % R, lambda R=R: numpy_search(R)), ('device_R%d' % R, lambda R=R: device_search(R))]
    object_loop(min(runs, 5))                                     # warm-up: every path, the device at every timed shape
    for R in args.replicas:
        numpy_search(R, min(runs, 2))
        device_search(R)
    times = {name: [] for name, _ in pieces}
    for r in range(args.repeats):
        k = r % len(pieces)
        for name, fn in pieces[k:] + pieces[:k]:                  # the order rotates from repeat to repeat
            times[name].append(fn())
    result = dict(envs=M, expansions=runs, depth=D, replicas=list(args.replicas), repeats=args.repeats, object_loop_envs_timed=K,
                  device=torch.cuda.get_device_name(0), gcn_arch=torch.cuda.get_device_properties(0).gcnArchName, host_cpus=len(os.sched_getaffinity(0)),
                  unit='ms per planning step of the whole batch (all expansions of all trees)')
    for name, _ in pieces:
        v = np.array(times[name]) * 1e3
        result[name] = dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))
        print('%-14s %12.3f ms (%.3f .. %.3f)' % (name, result[name]['median'], result[name]['min'], result[name]['max']), flush=True)
    # ---- one short episode batch: the search against the random policy
    episode = {}
    for policy in ('random', 'env_mcts'):
        np.random.seed(0)
        out = play(None, BatchedAvoidance.from_tasks(make(), device=dev), run_len=args.episode_len, mcts_steps=runs, max_rollout_depth=D,
                   policy=policy)
        episode[policy] = dict(summed_return=float(out['rewards'].sum()), mean_reward_per_step=float(out['rewards'].mean()))
        print('episode %-9s summed return %.0f over %d environments x %d steps' % (policy, episode[policy]['summed_return'], M, args.episode_len))
    result['episode'] = dict(envs=M, steps=args.episode_len, replicas=1, **episode)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
