#!/usr/bin/env python
"""Time the batched tree search on the learned model at the reference's default planning shape (100 trees, 100 expansions per tree,
rollout depth 10, 9 actions): BatchedMCTSHandler.run_mcts with fused=True (one ops.plan_expand per expansion) against fused=False
(the composed path: two Stove.rollout calls per expansion, entry points older than the fused one) and against handler.device_trees = True (the
trees on the device too: one ops.plan_search call for all expansions, forest uploaded before and downloaded after).

    python tools/plan_bench.py [--trees 100 --steps 100 --depth 10 --repeats 7 --out profiles/plan_bench.json]

Per mode and repeat: wall time of run_mcts (it ends in a device-to-host copy of q, so the device has finished), split by the handler
into host tree time (select, slot allocation, backpropagate) and device time (uploads, launches, waiting for q; the device-resident search reports its whole call as
device time).  The three modes alternate inside one process, after a warm-up run of each; the spread of the repeats is printed next to the median.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_model(dev):
    from stove_amd.video_prediction.config import StoveConfig
    from stove_amd.video_prediction.stove import Stove
    cfg = StoveConfig()
    cfg.num_obj, cfg.width, cfg.height = 3, 32, 32
    cfg.device, cfg.dtype, cfg.random_seed = dev, torch.float32, 42
    cfg.action_conditioned, cfg.action_space, cfg.debug_core_appearance = True, 9, True
    torch.manual_seed(0)
    return Stove(cfg).to(dev)


MODES = ('fused', 'composed', 'device_trees')


def one_run(model, z, app, depth, steps, mode, seed):
    from stove_amd.mcts.mcts_stove import MCTS, BatchedMCTSHandler
    trees = [MCTS(app[m:m + 1], z[m:m + 1], action_space=9, max_rollout_depth=depth) for m in range(z.shape[0])]
    h = BatchedMCTSHandler(trees, app, action_space=9, max_rollout_depth=depth)
    h.device_trees = mode == 'device_trees'
    np.random.seed(seed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    actions = h.run_mcts(model, steps, fused=mode != 'composed')
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    return actions, dict(total=total, host=h.timing['host'], device=h.timing['device'], min_gap=h.forest.min_gap)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--trees', type=int, default=100)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--depth', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'plan_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('plan_bench.py measures on a GPU; none found')
    dev = torch.device('cuda:0')
    model = build_model(dev)
    g = torch.Generator().manual_seed(1)
    z = torch.cat([torch.rand(args.trees, 3, 2, generator=g) * 0.2 + 0.1, torch.rand(args.trees, 3, 16, generator=g) * 1.2 - 0.6], -1)
    app = torch.rand(args.trees, 3, 3, generator=g)
    for mode in MODES:                                            # warm-up: every shape of the timed runs
        one_run(model, z, app, args.depth, min(args.steps, 5), mode, 0)
    runs = {mode: [] for mode in MODES}
    agree = True
    for r in range(args.repeats):
        acts = {}
        for mode in MODES[r % 3:] + MODES[:r % 3]:               # the order rotates from repeat to repeat
            acts[mode], rec = one_run(model, z, app, args.depth, args.steps, mode, 100 + r)
            runs[mode].append(rec)
        agree = agree and acts['fused'] == acts['composed'] == acts['device_trees']
    result = dict(trees=args.trees, steps=args.steps, depth=args.depth, actions=9, repeats=args.repeats, same_actions=agree,
                  device=torch.cuda.get_device_name(0), unit='ms per expansion (all trees)')
    for name in MODES:
        rec = {}
        for k in ('total', 'host', 'device'):
            v = np.array([x[k] for x in runs[name]]) * 1e3 / args.steps
            rec[k] = dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))
        rec['min_gap'] = float(min(x['min_gap'] for x in runs[name]))
        result[name] = rec
        print('%-12s per expansion: total %.3f ms (%.3f .. %.3f)  host tree %.3f ms (%.3f .. %.3f)  device %.3f ms (%.3f .. %.3f)' % (
            name, *[rec[k][s] for k in ('total', 'host', 'device') for s in ('median', 'min', 'max')]))
    print('same actions in all modes:', agree)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
