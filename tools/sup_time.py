"""Time one training step of the state-supervised baseline, composed against fused -> profiles/sup_rollout.json.

One step = SupTrainer.train_step on one batch: the rollout (V - 1 teacher-forced and R free steps), the loss, the backward and the
arena's one-launch Adam.  Two trainers of the same build in the same process, the same weights and batch:

  composed   SupervisedDynamics.forward(fused=False): V - 1 + R ops.gnn_step launches under autograd, as many backward
  fused      SupervisedDynamics.forward(fused=True): ops.sup_rollout, one launch each way plus the weight-gradient reduction

Shapes: B = 256, V = 6, R = 8 (the reference's training shape) at (N, cl) = (3, 16), (6, 16), (3, 64).  Also the 500-step no-grad
rollout of SupTrainer.long_rollout at B = 256, N = 3, cl = 16, both ways.  Events on the current stream around one call, 5 warm-up
calls each, median of 21, the variants alternating (one repetition of each per round); quartiles, min and max are kept.

`decision`: whether fused=None should resolve to the fused path -- true only if, at the reference's training shape, the fused path's
upper quartile lies below the composed path's lower quartile.  stove_amd/supairvised/dynamics.py: FUSED_DEFAULT carries the decision.

    python tools/sup_time.py [--out profiles/sup_rollout.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import numpy as np                                            # noqa: E402
import torch                                                  # noqa: E402

from rollout_sample_time import time_alternating             # noqa: E402


def trainer(n_obj, cl, B, V, R, dev):
    from stove_amd.supairvised.config import SupStoveConfig
    from stove_amd.supairvised.supstove import SupStove
    from stove_amd.supairvised.train import SupTrainer
    from stove_amd.video_prediction.load_data import StoveDataset
    c = SupStoveConfig()
    c.cl, c.num_obj, c.num_visible, c.num_rollout, c.batch_size = cl, n_obj, V, R, B
    c.device, c.dtype, c.random_seed, c.nolog = dev, torch.float32, 42, True
    c.action_conditioned, c.action_space = False, None
    c.experiment_dir, c.frame_store, c.num_workers = tempfile.mkdtemp(prefix='sup_time_'), 'f32', 0
    rs = np.random.RandomState(0)
    T = V + R
    y = np.concatenate([10.0 * rs.rand(B, T, n_obj, 2), 2.0 * rs.rand(B, T, n_obj, 2) - 1.0], -1)
    ds = StoveDataset(c, data={'X': np.zeros((B, T, 4, 4, 3), dtype=np.float32), 'y': y})
    c.num_frames, c.width, c.height, c.coord_lim, c.r = T, 4, 4, 10, 1.2
    torch.manual_seed(0)
    return SupTrainer(c, SupStove(c).to(dev), ds, ds)


def step_variants(n_obj, cl, B, V, R, dev):
    from stove_amd.supairvised import dynamics as SD
    fns, losses = {}, {}
    for name, fused in (('composed', False), ('fused', True)):
        tr = trainer(n_obj, cl, B, V, R, dev)
        data = next(iter(tr.dataloader))
        lat = torch.randn(B, n_obj, cl - 4, device=dev, generator=torch.Generator(dev).manual_seed(1))

        def fn(tr=tr, data=data, lat=lat, fused=fused):
            SD.FUSED_DEFAULT = fused
            return tr.train_step(data, latent=lat)[0]
        losses[name] = float(fn())
        fns[name] = fn
    assert abs(losses['composed'] - losses['fused']) <= 1e-5 * abs(losses['composed']), losses          # same weights, batch and latent
    return fns


def rollout_variants(n_obj, cl, B, V, num, dev):
    tr = trainer(n_obj, cl, B, V, 8, dev)
    x = next(iter(tr.dataloader))['present_labels']
    lat = torch.randn(B, n_obj, cl - 4, device=dev)

    def run(fused):
        def fn():
            with torch.no_grad():
                return tr.stove.dyn(x, num_rollout=num, fused=fused, latent=lat)[0]
        return fn
    fns = {'composed': run(False), 'fused': run(True)}
    assert torch.equal(fns['composed'](), fns['fused']())
    return fns


def rows_of(times):
    def row(v):
        q = statistics.quantiles(v, n=4)
        return dict(ms=statistics.median(v), q1_ms=q[0], q3_ms=q[2], min_ms=min(v), max_ms=max(v))
    return {k: row(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sup_rollout.json'))
    ap.add_argument('--batch', type=int, default=256)
    args = ap.parse_args()
    from stove_amd import build
    build.build_library()
    from stove_amd.supairvised import dynamics as SD
    default = SD.FUSED_DEFAULT
    dev = torch.device('cuda:0')
    B, V, R = args.batch, 6, 8
    steps = {}
    for n_obj, cl in ((3, 16), (6, 16), (3, 64)):
        rows = rows_of(time_alternating(step_variants(n_obj, cl, B, V, R, dev)))
        steps['N%d_cl%d' % (n_obj, cl)] = dict(rows=rows, speedup_fused_over_composed=rows['composed']['ms'] / rows['fused']['ms'])
        print(n_obj, cl, rows, flush=True)
    SD.FUSED_DEFAULT = default
    long_rows = rows_of(time_alternating(rollout_variants(3, 16, B, V, 500, dev), warm=3, reps=11))
    print('long rollout', long_rows, flush=True)
    ref = steps['N3_cl16']['rows']
    faster = ref['fused']['q3_ms'] < ref['composed']['q1_ms']
    result = dict(device=torch.cuda.get_device_name(0), B=B, V=V, R=R, source_hash=build.source_hash(),
                  method='hip events around one call, 5 warm-up calls, median of 21 (long rollout: 3 and 11), the variants alternating; '
                         'train_step = rollout + loss + backward + one-launch Adam on one resident batch with a fed latent; '
                         'composed = fused=False (a launch per step each way), fused = ops.sup_rollout',
                  train_step=steps,
                  long_rollout_500=dict(rows=long_rows, speedup_fused_over_composed=long_rows['composed']['ms'] / long_rows['fused']['ms']),
                  decision=dict(fused_default=bool(faster), shipped_default=bool(default),
                                rule='fused=None resolves to the fused path iff its upper quartile at N = 3, cl = 16 lies below the '
                                     'composed path\'s lower quartile'))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps({k: {r: round(v['ms'], 3) for r, v in s['rows'].items()} for k, s in steps.items()}), result['decision'])


if __name__ == '__main__':
    main()
