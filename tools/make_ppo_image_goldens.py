"""Record the reference's PPO arm on images for tests/test_ppo_image_cpu.py: tests/golden/g26_ppo_images.npz and
g26_reference_fp32_gap.json.

    python tools/make_ppo_image_goldens.py --reference /path/to/the/reference/checkout

The stand-ins and the import-not-copy rule are those of tools/make_ppo_goldens.py, whose loader this script uses: nothing of the
reference's text is copied, its classes are imported from the checkout, run, and their inputs and outputs written down.

Per case c of (F, H, deep) = (4, 16, False), (2, 8, True), on BillardsEnv(n=3, granularity=2, seed=60 + c) under
AvoidanceTask(num_stacked=F, action_force=.3), main_rl's settings:
  c{c}_sd_<key>                  the state_dict of Policy((32, 32, 3F), 9, hidden_size=H, stacked_frames=F, use_deep_layers=deep) under
                                 torch.manual_seed(200 + c)
  c{c}_warm (4, 32, 32, 3F) f64  the frame buffer after each of the four step_frame_buffer(0) that follow env.reset() and the zeroing
                                 of the buffer (rows that no frame has reached yet are zero)
  c{c}_buf (4, 32, 32, 3F) f64   the buffer Runner.reset(frame_buffer=True) returns on a fresh environment of the same seed (== warm[3]),
                                 then after three further step_frame_buffer(a) with a = c{c}_buf_actions
  c{c}_x, c{c}_v (4, 3, 2) f64   the states that go with those four buffers
  c{c}_actions (4,)              the actions evaluated
  c{c}_value, logits, eval_value, eval_logp, eval_entropy + '64' / '32'     the reference policy's outputs on the four buffers (permuted
                                 to channels first, as its runner feeds them) in float64 and in float32
The json holds, per case, the largest deviation of the reference's own float32 outputs from its float64 outputs."""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((4, 16, False), (2, 8, True))
BUF_ACTIONS = ((3, 0, 7), (5, 2, 8))
ACTIONS = ((1, 4, 0, 8), (6, 2, 2, 7))


def _loader():
    spec = importlib.util.spec_from_file_location('make_ppo_goldens', os.path.join(ROOT, 'tools', 'make_ppo_goldens.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.load_reference


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True)
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    args = ap.parse_args()
    rl_model, agents, runners, envs = _loader()(args.reference)
    G, gap = {'cases': np.int32(len(SHAPES))}, {}
    for c, (F, H, deep) in enumerate(SHAPES):
        pre = 'c%d_' % c
        make = lambda: envs.AvoidanceTask(envs.BillardsEnv(n=3, granularity=2, seed=60 + c), num_stacked=F, action_force=.3)
        # ---- the buffer while it fills
        task = make()
        task.env.reset()
        task.frame_buffer[:] = 0.
        G[pre + 'warm'] = np.stack([task.step_frame_buffer(0)[0].copy() for _ in range(4)])
        # ---- reset(frame_buffer=True), then three steps
        task = make()
        runner = object.__new__(runners.Runner)
        runner.env, runner.task = task.env, task
        bufs, xs, vs = [], [], []

        def keep(result):
            bufs.append(result[0].copy())
            xs.append(task.env.x.copy())
            vs.append(task.env.v.copy())
        keep(runner.reset(frame_buffer=True))
        for a in BUF_ACTIONS[c]:
            keep(task.step_frame_buffer(a))
        G[pre + 'buf'], G[pre + 'x'], G[pre + 'v'] = np.stack(bufs), np.stack(xs), np.stack(vs)
        G[pre + 'buf_actions'] = np.array(BUF_ACTIONS[c], dtype=np.int64)
        assert G[pre + 'buf'].shape == (4, 32, 32, 3 * F) and np.array_equal(G[pre + 'buf'][0], G[pre + 'warm'][3])
        # ---- the policy on them
        torch.manual_seed(200 + c)
        policy = rl_model.Policy(task.get_framebuffer_shape(), 9, hidden_size=H, stacked_frames=F, use_deep_layers=deep)
        for k, ten in policy.state_dict().items():
            G[pre + 'sd_' + k] = ten.numpy().copy()
        actions = np.array(ACTIONS[c], dtype=np.int64).reshape(4, 1)
        G[pre + 'actions'] = actions[:, 0]
        res = {}
        for tag, dt in (('32', torch.float32), ('64', torch.float64)):
            p = policy.to(dt)
            o = torch.from_numpy(G[pre + 'buf']).to(dt).permute(0, 3, 1, 2).contiguous()
            with torch.no_grad():
                value, dist = p.head(p.base(o))
                ev, elp, ent = p.evaluate_actions(o, torch.from_numpy(actions))
            res[tag] = {'value': value, 'logits': dist.logits, 'eval_value': ev, 'eval_logp': elp, 'eval_entropy': ent}
            for k, ten in res[tag].items():
                G[pre + k + tag] = ten.numpy().copy()
        gap['case%d' % c] = {'shape': [F, H, bool(deep)],
                             **{k: float((res['32'][k].double() - res['64'][k]).abs().max())
                                for k in ('value', 'logits', 'eval_logp', 'eval_entropy')}}
    np.savez_compressed(os.path.join(args.out, 'g26_ppo_images.npz'), **G)
    with open(os.path.join(args.out, 'g26_reference_fp32_gap.json'), 'w') as fh:
        json.dump(gap, fh, indent=1, sort_keys=True)
    print(json.dumps(gap, indent=1, sort_keys=True))
    print(os.path.getsize(os.path.join(args.out, 'g26_ppo_images.npz')), 'bytes')


if __name__ == '__main__':
    main()
