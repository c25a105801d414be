#!/usr/bin/env python
"""Time the batched tree search on the learned model at the reference's default planning shape (100 trees, 100 expansions per tree,
rollout depth 10, 9 actions): BatchedMCTSHandler.run_mcts with fused=True (one ops.plan_expand per expansion) against fused=False
(the composed path: two Stove.rollout calls per expansion, entry points older than the fused one) and against handler.device_trees = True (the
trees on the device too: one ops.plan_search call for all expansions, forest uploaded before and downloaded after).

    python tools/plan_bench.py [--trees 100 --steps 100 --depth 10 --repeats 7 --cl 32 --out profiles/plan_bench.json]

--cl 16 / 64: the same on a model of that state-code length, the handler's fused_widths switched on for it; the result goes under the
key 'cl16' / 'cl64' of profiles/plan_bench_cl.json, next to the other width's.

Per mode and repeat: wall time of run_mcts (it ends in a device-to-host copy of q, so the device has finished), split by the handler
into host tree time (select, slot allocation, backpropagate) and device time (uploads, launches, waiting for q; the device-resident search reports its whole call as
device time).  The three modes have to return the same actions in every repeat.  A tree on which the composed search ends elsewhere is traced
afterwards, untimed (trace_difference: the iteration and the decision at which the two searches part, the two candidates' Qsa and UCT
values under both); 'same_actions_where_decided' is false unless every such decision lies between candidates less than DECIDED_GAP apart.
The three modes alternate inside one process, after a warm-up run of each; the spread of the repeats is printed next to the median.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_model(dev, cl=32):
    from stove_amd.video_prediction.config import StoveConfig
    from stove_amd.video_prediction.stove import Stove
    cfg = StoveConfig()
    cfg.num_obj, cfg.width, cfg.height = 3, 32, 32
    cfg.device, cfg.dtype, cfg.random_seed = dev, torch.float32, 42
    cfg.action_conditioned, cfg.action_space, cfg.debug_core_appearance = True, 9, True
    if cl != 32:
        cfg.cl, cfg.transition_lik_std = cl, [0.01] * (cl // 2)
    torch.manual_seed(0)
    return Stove(cfg).to(dev)


MODES = ('fused', 'composed', 'device_trees')


def one_run(model, z, app, depth, steps, mode, seed):
    from stove_amd.mcts.mcts_stove import MCTS, BatchedMCTSHandler
    trees = [MCTS(app[m:m + 1], z[m:m + 1], action_space=9, max_rollout_depth=depth) for m in range(z.shape[0])]
    h = BatchedMCTSHandler(trees, app, action_space=9, max_rollout_depth=depth)
    h.device_trees = mode == 'device_trees'
    if model.c.cl != 32:
        h.fused_widths = (model.c.cl,)
    np.random.seed(seed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    actions = h.run_mcts(model, steps, fused=mode != 'composed')
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    return actions, dict(total=total, host=h.timing['host'], device=h.timing['device'], min_gap=h.forest.min_gap)


def walk(f, m):
    """Forest.select for tree m alone, without changing anything: per level a dict of the node, the best value carried in from the
    levels above, the UCT values, Qsa and Nsa of its A children, and the action taken"""
    cur, cur_best, best_act, levels = 0, -np.inf, 0, []
    while f.first[m, cur] >= 0 and f.depth[m, cur] + 1 != f.D:
        ch = f.first[m, cur] + np.arange(f.A)
        with np.errstate(divide='ignore', invalid='ignore'):
            u = f.Qsa[m, ch] + f.c * np.sqrt(np.log(f.Ns[m, cur]) / (1 + f.Nsa[m, ch]))
        carried = cur_best
        for a in range(f.A):
            if u[a] > cur_best:
                cur_best, best_act = u[a], a
        levels.append(dict(node=int(cur), carried=float(carried), u=u.copy(), Qsa=f.Qsa[m, ch].copy(), Nsa=f.Nsa[m, ch].copy(), taken=int(best_act)))
        cur = int(f.first[m, cur] + best_act)
    return levels


def searched(model, z, app, depth, steps, fused, acts):
    """an untimed host search on given rollout actions -> (actions, the leaf selected per iteration (steps, trees), the forest)"""
    from stove_amd.mcts.mcts_stove import MCTS, BatchedMCTSHandler
    trees = [MCTS(app[m:m + 1], z[m:m + 1], action_space=9, max_rollout_depth=depth) for m in range(z.shape[0])]
    h = BatchedMCTSHandler(trees, app, action_space=9, max_rollout_depth=depth)
    if model.c.cl != 32:
        h.fused_widths = (model.c.cl,)
    leaves, select = [], h.forest.select

    def recording_select():
        leaf = select()
        leaves.append(leaf.copy())
        return leaf
    h.forest.select = recording_select
    actions = h.run_mcts(model, steps, fused=fused, rollout_actions=acts[:steps])
    return actions, np.stack(leaves) if leaves else np.zeros((0, z.shape[0]), dtype=np.int64), h.forest


# The margin at which the fused and the composed search have to take the same decision: tests/plan_cases.py SEARCH_GAP, what
# tests/test_gpu_plan_search.py and tests/test_gpu_plan_cl.py require of every decision before they compare the two.  The two expansions
# round differently -- the fused one forms q in float32 (spacing 7.6e-6 at |q| = 74, the benchmark's depth), the composed one in float64
# from float32 rewards of another order of operations -- so candidates closer than this may rank either way.
DECIDED_GAP = 1e-4


def trace_difference(model, z, app, depth, steps, seed, m, want):
    """Why tree m of the repeat drawn from `seed` ends on another action under the composed search than under the fused one: both
    searches again, untimed, on the same rollout actions; the first iteration at which they select different leaves; both forests as
    they stand before that iteration; the level of tree m's walk at which the two take different children, with the two children's
    Qsa, Nsa and UCT values under both searches.  `decided`: whether either search holds the two at least DECIDED_GAP apart; the gaps are also
    given in float32 spacings of the Qsa compared."""
    np.random.seed(seed)
    acts = np.stack([np.random.randint(9, size=(9 * z.shape[0] * depth * 2,)) for _ in range(steps)])
    runs = {name: searched(model, z, app, depth, steps, name == 'fused', acts) for name in ('fused', 'composed')}
    out = dict(tree=int(m), seed=int(seed), reproduced=all(runs[k][0][m] == want[k] for k in runs),
               actions={k: int(runs[k][0][m]) for k in runs})
    apart = np.flatnonzero(runs['fused'][1][:, m] != runs['composed'][1][:, m])
    if not apart.size:
        return dict(out, iteration=None, decided=None)
    it = int(apart[0])
    before = {k: searched(model, z, app, depth, it, k == 'fused', acts)[2] for k in runs}
    walks = {k: walk(before[k], m) for k in runs}
    level = next((i for i, (a, b) in enumerate(zip(walks['fused'], walks['composed'])) if a['taken'] != b['taken'] or a['node'] != b['node']), None)
    if level is None:
        return dict(out, iteration=it, level=None, decided=None)
    lf, lc = walks['fused'][level], walks['composed'][level]
    pair = (lf['taken'], lc['taken'])
    out.update(iteration=it, level=level, node=lf['node'], same_node=lf['node'] == lc['node'], children=[int(a) for a in pair],
               same_visit_counts=bool(np.array_equal(lf['Nsa'], lc['Nsa'])))
    scale = 0.0
    for k, lv in (('fused', lf), ('composed', lc)):
        out[k] = dict(Qsa=[float(lv['Qsa'][a]) for a in pair], Nsa=[int(lv['Nsa'][a]) for a in pair], uct=[float(lv['u'][a]) for a in pair],
                      carried=lv['carried'] if np.isfinite(lv['carried']) else None, gap=float(abs(lv['u'][pair[0]] - lv['u'][pair[1]])))
        scale = max(scale, float(np.abs(lv['Qsa'][list(pair)]).max()))
    out['float32_spacing_of_Qsa'] = float(np.spacing(np.float32(scale)))
    for k in ('fused', 'composed'):
        out[k]['gap_in_float32_spacings'] = out[k]['gap'] / out['float32_spacing_of_Qsa']
    out['decided_gap'] = DECIDED_GAP
    out['decided'] = bool(max(out['fused']['gap'], out['composed']['gap']) >= DECIDED_GAP)
    return out


def kernel_times(model, z, app, depth, iters):
    """device time per kernel of the device-resident search, by torch.profiler over one search of `iters` expansions after a warm-up
    -> {kernel name: dict(ms per expansion, launches per expansion)}, the largest first"""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    one_run(model, z, app, depth, iters, 'device_trees', 0)
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        one_run(model, z, app, depth, iters, 'device_trees', 1)
        torch.cuda.synchronize()
    out = {}
    for e in prof.key_averages():
        t = getattr(e, 'device_time_total', None)
        t = getattr(e, 'cuda_time_total', 0) if t is None else t
        if e.device_type == DeviceType.CUDA and t > 0:
            out[e.key.split('(')[0]] = dict(ms=t / 1e3 / iters, launches=e.count / iters)
    return dict(sorted(out.items(), key=lambda kv: -kv[1]['ms']))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--trees', type=int, default=100)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--depth', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--cl', type=int, default=32, choices=(16, 32, 64), help='state-code length of the model')
    ap.add_argument('--out', default=None, help='default: profiles/plan_bench.json, at --cl 16 / 64 profiles/plan_bench_cl.json')
    ap.add_argument('--kernels', default=None, metavar='JSON', help='instead of timing the modes: device time per kernel of a '
                    'device-resident search of 20 expansions (torch.profiler), into the key cl<N> of this file')
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, 'profiles', 'plan_bench.json' if args.cl == 32 else 'plan_bench_cl.json')
    if not torch.cuda.is_available():
        raise SystemExit('plan_bench.py measures on a GPU; none found')
    dev = torch.device('cuda:0')
    model = build_model(dev, args.cl)
    g = torch.Generator().manual_seed(1)
    z = torch.cat([torch.rand(args.trees, 3, 2, generator=g) * 0.2 + 0.1, torch.rand(args.trees, 3, args.cl // 2, generator=g) * 1.2 - 0.6], -1)
    app = torch.rand(args.trees, 3, 3, generator=g)
    if args.kernels:
        whole = {}
        if os.path.exists(args.kernels):
            with open(args.kernels) as f:
                whole = json.load(f)
        whole['cl%d' % args.cl] = dict(trees=args.trees, depth=args.depth, expansions=20, unit='ms per expansion (all trees)',
                                       device=torch.cuda.get_device_name(0), kernels=kernel_times(model, z, app, args.depth, 20))
        with open(args.kernels, 'w') as f:
            json.dump(whole, f, indent=1, sort_keys=True)
            f.write('\n')
        print(json.dumps(whole['cl%d' % args.cl]))
        return
    for mode in MODES:                                            # warm-up: every shape of the timed runs
        one_run(model, z, app, args.depth, min(args.steps, 5), mode, 0)
    runs = {mode: [] for mode in MODES}
    agree, agreed, differ, traces = True, [], {'composed': [], 'device_trees': []}, []
    for r in range(args.repeats):
        acts = {}
        for mode in MODES[r % 3:] + MODES[:r % 3]:               # the order rotates from repeat to repeat
            acts[mode], rec = one_run(model, z, app, args.depth, args.steps, mode, 100 + r)
            runs[mode].append(rec)
        agreed.append(acts['fused'] == acts['composed'] == acts['device_trees'])
        for mode in differ:                                       # trees whose action is not the fused search's
            differ[mode].append(sum(a != b for a, b in zip(acts[mode], acts['fused'])))
        agree = agree and agreed[-1]
        for m in range(args.trees):                               # a composed search that ends elsewhere: traced to the decision, untimed
            if acts['composed'][m] != acts['fused'][m]:
                traces.append(dict(trace_difference(model, z, app, args.depth, args.steps, 100 + r, m,
                                                    {k: acts[k][m] for k in ('fused', 'composed')}), repeat=r))
    # the device search runs the fused search's arithmetic and has to agree with it outright; the composed search rounds its rewards
    # differently and has to agree wherever the candidates are DECIDED_GAP apart (trace_difference)
    decided = all(n == 0 for n in differ['device_trees']) and all(t['decided'] is False and t['reproduced'] for t in traces)
    result = dict(cl=args.cl, same_actions_per_repeat=agreed, trees_differing_from_fused=differ, trees=args.trees, steps=args.steps,
                  depth=args.depth, actions=9, repeats=args.repeats, same_actions=agree, same_actions_where_decided=decided,
                  differences_traced=traces,
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
    print('same actions in all modes:', agree, ' wherever the candidates are %g apart:' % DECIDED_GAP, decided)
    for t in traces:
        print('traced:', json.dumps(t))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    whole = result
    if args.cl != 32:                                             # one file for the widths other than 32, a key per width
        whole = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                whole = json.load(f)
        whole['cl%d' % args.cl] = result
    with open(args.out, 'w') as f:
        json.dump(whole, f, indent=1, sort_keys=args.cl != 32)
        f.write('\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
