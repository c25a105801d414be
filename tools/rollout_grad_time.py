"""Time forward + backward through Stove.rollout the ways it can run under autograd -> profiles/rollout_grad.json.

B = 256, N = 3 and 6, num = 92, cl = 32, no noise_fn (the library's generator draws), all parameters trainable:

  fused_sample     Stove.rollout(sample=True, fused=True): one draw, one launch forward (stove_rollout_sample_fwd), one launch backward
                   (stove_rollout_bwd) plus the fixed-order reduction of the weight gradients
  step_loop        Stove.rollout(sample=True, fused=None) under autograd: the host loop of single differentiable steps -- the only
                   differentiable sampling path before the one-launch backward, and still the default
  fused_mean       Stove.rollout(sample=False) forward + backward
  fused_mean_fwd   the same forward alone, under autograd (what the backward adds is the difference)

Each timed call is forward, a loss (z_pred and, when sampling, log_q summed) and loss.backward(), with the parameters' .grad dropped
first.  Events on the current stream around one call, 5 warm-up calls each, median of 21; the variants are timed in alternation (one
repetition of each per round), so that whatever else the machine is doing falls on all of them alike; min and max are kept as the range.

    python tools/rollout_grad_time.py [--out profiles/rollout_grad.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import torch                                                  # noqa: E402

from rollout_sample_time import time_alternating             # noqa: E402


def variants(n_obj, B, num, dev):
    from stove_amd.video_prediction.config import StoveConfig
    from stove_amd.video_prediction.stove import Stove
    cfg = StoveConfig()
    cfg.num_obj, cfg.width, cfg.height = n_obj, 32, 32
    cfg.device, cfg.dtype, cfg.random_seed = dev, torch.float32, 42
    cfg.action_conditioned, cfg.action_space = False, None
    if n_obj != 3:
        cfg.debug_match_objects = 'greedy'
    torch.manual_seed(0)
    st = Stove(cfg).to(dev)
    z_last = torch.cat([torch.rand(B, n_obj, 2, device=dev) * 0.2 + 0.1, torch.rand(B, n_obj, 16, device=dev) - 0.5], -1)

    def run(sample, fused, backward=True):
        def fn():
            st.zero_grad(set_to_none=True)
            z0 = z_last.clone().requires_grad_()
            out = st.rollout(z0, num=num, sample=sample, fused=fused)
            if backward:
                loss = out[0].sum() + (out[1].sum() if sample else 0)
                loss.backward()
            return out[0], z0.grad
        return fn
    fns = {'fused_sample': run(True, True), 'step_loop': run(True, None), 'fused_mean': run(False, None),
           'fused_mean_fwd': run(False, None, backward=False)}
    for k, fn in fns.items():
        z, g = fn()
        assert z.shape == (B, num, n_obj, 18) and bool(torch.isfinite(z).all()), k
        assert (g is None) == (k == 'fused_mean_fwd') and (g is None or bool(torch.isfinite(g).all())), k
    return fns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rollout_grad.json'))
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--objects', type=int, nargs='+', default=[3, 6])
    ap.add_argument('--steps', type=int, default=92)
    args = ap.parse_args()
    from stove_amd import build
    build.build_library()
    dev = torch.device('cuda:0')
    B, num = args.batch, args.steps
    shapes = {}
    for n_obj in args.objects:
        times = time_alternating(variants(n_obj, B, num, dev))
        rows = {}
        for k, v in times.items():
            med = statistics.median(v)
            rows[k] = dict(ms=med, us_per_step=1e3 * med / num, min_ms=min(v), max_ms=max(v))
            print(n_obj, k, rows[k], flush=True)
        shapes['N%d' % n_obj] = dict(rows=rows, speedup_fused_sample_over_step_loop=rows['step_loop']['ms'] / rows['fused_sample']['ms'],
                                     backward_of_fused_mean_ms=rows['fused_mean']['ms'] - rows['fused_mean_fwd']['ms'])
    result = dict(device=torch.cuda.get_device_name(0), B=B, num=num, cl=32, source_hash=build.source_hash(),
                  method='hip events around one call = Stove.rollout + loss + backward (fused_mean_fwd: the forward alone), parameters '
                         'trainable, 5 warm-up calls, median of 21, the variants alternating; fused_sample = sample=True, fused=True; '
                         'step_loop = sample=True, fused=None (host loop of single steps); fused_mean = sample=False',
                  shapes=shapes)
    with open(args.out, 'w') as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps({k: {r: round(v['ms'], 3) for r, v in s['rows'].items()} for k, s in shapes.items()}))


if __name__ == '__main__':
    main()
