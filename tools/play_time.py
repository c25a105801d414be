#!/usr/bin/env python
"""Time the pieces of one closed-loop planning step (stove_amd/mcts/play.py) at the reference's shape: 100 avoidance environments
(n = 3, hw = 10, r = 1, res = 32, granularity 5), 100 expansions per tree, rollout depth 10.

    python tools/play_time.py [--envs 100 --steps 100 --depth 10 --repeats 7 --env-steps 20 --out profiles/play.json]

Per environment step of the batch, in ms:
  host_loop    stepping and drawing the AvoidanceTask objects one by one (what the reference's loop does), frames stacked as float64
  numpy_batch  BatchedAvoidance(device=None).step: numpy over the batch
  device_batch BatchedAvoidance(device='cuda:0').step: one stove_env_step launch, ended by a device synchronise
  encode       the model's inference pass on the 8-frame ring, as plan_on_frames runs it before the search (ring already on the device)
  encode_host  the same from a float64 numpy ring on the host (encode_img + upload), as plan_on_model runs it
  search       `steps` expansions per tree, composed path (the default of run_mcts) and device_trees=True
The pieces run in one process after a warm-up of each, in an order that rotates from repeat to repeat; median and range of the
repeats are reported.  Every timed piece ends in a device synchronise or a device-to-host copy.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.plan_bench import build_model  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=100)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--depth', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--env-steps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'play.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('play_time.py measures on a GPU; none found')
    from stove_amd.envs import envs
    from stove_amd.envs.batched import BatchedAvoidance
    from stove_amd.mcts.mcts_stove import MCTS, BatchedMCTSHandler, encode_img
    from stove_amd.mcts.play import warm_up
    dev = torch.device('cuda:0')
    M, K = args.envs, args.env_steps
    model = build_model(dev)
    tasks = [envs.AvoidanceTask(envs.BillardsEnv(n=3, hw=10, r=1., res=32, seed=s), action_force=0.6) for s in range(M)]
    host = BatchedAvoidance.from_tasks(tasks)
    device = BatchedAvoidance.from_tasks(tasks, device=dev)
    rings = warm_up(BatchedAvoidance.from_tasks(tasks, device=dev))
    x_dev, a_dev = rings.tensors()
    x_host = np.transpose(x_dev.cpu().numpy().astype(np.float64), (0, 1, 3, 4, 2))          # the layout initialize_img keeps
    rs = np.random.RandomState(0)

    def host_loop():
        acts = rs.randint(9, size=(K, M))
        t0 = time.perf_counter()
        for k in range(K):
            np.stack([tasks[j].step(int(acts[k, j]))[0] for j in range(M)])
        return (time.perf_counter() - t0) / K

    def numpy_batch():
        acts = rs.randint(9, size=(K, M))
        t0 = time.perf_counter()
        for k in range(K):
            host.step(acts[k])
        return (time.perf_counter() - t0) / K

    def device_batch():
        acts = torch.from_numpy(rs.randint(9, size=(K, M)).astype(np.int32)).to(dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(K):
            device.step(acts[k])
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) / K

    def infer(x):
        with torch.no_grad():
            _, prop, _ = model(x.to(dev), 0, actions=a_dev, pretrain=False)
        return prop

    def encode():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        infer(x_dev)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def encode_host():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        infer(encode_img(x_host))
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    prop = infer(x_dev)
    z, app = prop['z'][:, -1].clone(), prop['obj_appearances'][:, -1].clone()

    def search(device_trees, steps=None):
        trees = [MCTS(app[m:m + 1], z[m:m + 1], max_rollout_depth=args.depth) for m in range(M)]
        h = BatchedMCTSHandler(trees, app, action_space=9, max_rollout_depth=args.depth)
        h.device_trees = device_trees
        np.random.seed(5)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            h.run_mcts(model, args.steps if steps is None else steps)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    pieces = [('host_loop', host_loop), ('numpy_batch', numpy_batch), ('device_batch', device_batch), ('encode', encode),
              ('encode_host', encode_host), ('search_composed', lambda: search(False)), ('search_device_trees', lambda: search(True))]
    for name, fn in pieces:                                       # warm-up: every shape of the timed runs
        if name.startswith('search'):
            search(name == 'search_device_trees', min(args.steps, 5))
        else:
            fn()
    runs = {name: [] for name, _ in pieces}
    for r in range(args.repeats):
        k = r % len(pieces)
        for name, fn in pieces[k:] + pieces[:k]:                  # the order rotates from repeat to repeat
            runs[name].append(fn())
    result = dict(envs=M, expansions=args.steps, depth=args.depth, repeats=args.repeats, env_steps_per_repeat=K,
                  device=torch.cuda.get_device_name(0), host_cpus=len(os.sched_getaffinity(0)),
                  unit='ms per environment step of the whole batch (search: ms per planning step, all expansions)')
    for name, _ in pieces:
        v = np.array(runs[name]) * 1e3
        result[name] = dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))
        print('%-20s %9.3f ms (%.3f .. %.3f)' % (name, result[name]['median'], result[name]['min'], result[name]['max']))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
