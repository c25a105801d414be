"""Time Trainer.pixel_error with the squared error fused into the render kernel against the materialising path ->
profiles/pixel_error.json.

Two shapes, 256 test sequences x 100 frames of seeded random pixels and labels (the time does not depend on what the frames show), 8
frames visible, 92 rolled out, 3 objects, untrained weights:

  headline   32 x 32, one channel (debug_bw), 10 x 10 glimpses
  colour50   50 x 50, three channels (debug_bw = False)
  large512   4 frames of 512 x 512, one channel, render rows only: where the fused launch (one workgroup per frame) stops paying

  fused      pixel_error(fused=True): stove_render_frames_any returns the per-frame squared error, no frame is written
  frames     pixel_error(fused=False): reconstruct_from_z materialises the frames, the mean is taken by torch ops
  render_*   the two render paths alone on the evaluation's own states and frames (what differs between the two calls; the
             encode and the rollout are common to both)

A whole call ends in a device-to-host copy of its result, so a host clock around it covers the device work; the render-only rows
use device events.  5 warm-up calls each, median of 21, the variants alternating within a round; min and max are kept as the range.

    python tools/pixel_error_time.py [--out profiles/pixel_error.json]
"""
import argparse
import json
import os
import pickle
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np                                             # noqa: E402
import torch                                                   # noqa: E402

SHAPES = {'headline': dict(res=32, colour=False), 'colour50': dict(res=50, colour=True)}


def make_trainer(tmp, name, res, colour, n_seq, t_len, visible):
    from stove_amd.main import main as build_trainer
    rng = np.random.RandomState(7)
    y = np.concatenate([rng.uniform(1, 9, (n_seq, t_len, 3, 2)), rng.uniform(-1, 1, (n_seq, t_len, 3, 2))], -1)
    data = {'X': rng.uniform(0, 1, (n_seq, t_len, res, res, 3)).astype(np.float32), 'y': y, 'coord_lim': 10, 'r': 1.2}
    path = os.path.join(tmp, name + '.pkl')
    with open(path, 'wb') as f:
        pickle.dump(data, f)
    args = {'traindata': path, 'testdata': path, 'nolog': 'True', 'experiment_dir': tmp, 'batch_size': str(n_seq),
            'num_visible': str(visible), 'num_rollout': '8', 'num_workers': '0', 'dtype': 'torch.float', 'random_seed': '42',
            'num_epochs': '1'}
    if colour:
        args.update(debug_bw='False', channels='3')
    return build_trainer(sh_args=args)


def time_alternating(fns, clock, warm=5, reps=21):
    """{name: callable} -> {name: [ms, ...]}: `reps` rounds, every callable once per round, each under clock(fn) -> ms"""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            out[k].append(clock(fn))
    return out


def host_clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def event_clock(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def rows_of(times):
    return {k: dict(ms=statistics.median(v), min_ms=min(v), max_ms=max(v)) for k, v in times.items()}


def measure(trainer):
    from stove_amd import ops
    c, sup = trainer.c, trainer.stove.sup
    whole = rows_of(time_alternating({'fused': lambda: trainer.pixel_error(fused=True),
                                      'frames': lambda: trainer.pixel_error(fused=False)}, host_clock))
    a, b = trainer.pixel_error(fused=True)['mse'], trainer.pixel_error(fused=False)['mse']
    # the render paths alone, on states of the evaluation's shape
    n, T = c.batch_size, c.num_frames // c.frame_step - c.skip
    g = torch.Generator().manual_seed(3)
    z = torch.cat([0.1 + 0.3 * torch.rand(n, T, 3, 2, generator=g), 1.8 * torch.rand(n, T, 3, 2, generator=g) - 0.9], -1).to(c.device)
    truth = torch.rand(n, T, c.channels, c.width, c.height, generator=g).to(c.device)
    bg, patches, per = sup.render_inputs(z)

    def fused():
        return ops.render_frames_any(bg, patches, per, z.view(-1, 4), 3, sup.render_geom(), truth=truth.view(n * T, -1), want_frames=False)[1]

    def frames():
        return torch.mean((truth - torch.clamp(sup.reconstruct_from_z(z), 0, 1)) ** 2, dim=(0, 2, 3, 4))
    alone = rows_of(time_alternating({'render_fused': fused, 'render_frames': frames}, event_clock))
    return dict(frames_scored=n * T, pixels_per_frame=c.channels * c.width * c.height, rows={**whole, **alone},
                fused_over_frames=whole['frames']['ms'] / whole['fused']['ms'],
                render_fused_over_frames=alone['render_frames']['ms'] / alone['render_fused']['ms'],
                mse_max_abs_diff=float((a.double() - b.double()).abs().max()))


def measure_large(res=512, n_frames=4, n_obj=3):
    """The fused launch's limit: with sqerr asked for a frame is ONE workgroup whatever its size, so a few large frames leave most of
    the device idle; the tiled render (one workgroup per 1024 positions) followed by a torch reduction is the alternative."""
    from stove_amd import ops
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(5)
    geom = (1, res, res, 10, 10, False)
    bg, patch = torch.rand(res * res, generator=g).to(dev), torch.rand(1, 100, generator=g).to(dev)
    z = torch.cat([0.1 + 0.3 * torch.rand(n_frames * n_obj, 2, generator=g), 1.8 * torch.rand(n_frames * n_obj, 2, generator=g) - 0.9], -1).to(dev)
    truth = torch.rand(n_frames, res * res, generator=g).to(dev)

    def fused():
        return ops.render_frames_any(bg, patch, 0, z, n_obj, geom, truth=truth, want_frames=False)[1]

    def tiled():
        return ((ops.render_frames_any(bg, patch, 0, z, n_obj, geom) - truth) ** 2).sum(1)
    rows = rows_of(time_alternating({'render_fused': fused, 'render_tiled_then_torch_sum': tiled}, event_clock))
    rel = float(((fused().double() - tiled().double()).abs() / tiled().double()).max())
    return dict(frames_scored=n_frames, pixels_per_frame=res * res, rows=rows, sqerr_max_rel_diff=rel,
                render_fused_over_tiled=rows['render_tiled_then_torch_sum']['ms'] / rows['render_fused']['ms'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pixel_error.json'))
    ap.add_argument('--sequences', type=int, default=256)
    ap.add_argument('--frames', type=int, default=100)
    ap.add_argument('--visible', type=int, default=8)
    args = ap.parse_args()
    from stove_amd import build
    build.build_library()
    if not torch.cuda.is_available():
        raise RuntimeError('pixel_error_time: no GPU, nothing to measure')
    shapes = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, kw in SHAPES.items():
            print(name, 'building the trainer', flush=True)
            trainer = make_trainer(tmp, name, kw['res'], kw['colour'], args.sequences, args.frames, args.visible)
            print(name, 'timing', flush=True)
            shapes[name] = measure(trainer)
            print(name, json.dumps(shapes[name]), flush=True)
            del trainer
            torch.cuda.empty_cache()
    shapes['large512'] = measure_large()
    print('large512', json.dumps(shapes['large512']), flush=True)
    result = dict(device=torch.cuda.get_device_name(0), sequences=args.sequences, frames=args.frames, visible=args.visible,
                  source_hash=build.source_hash(),
                  method='fused / frames: host clock around one Trainer.pixel_error call between device synchronisations (encode + rollout '
                         '+ render + score + position error); render_*: device events around the render-and-score part alone; 5 warm-up '
                         'calls, median of 21, the variants alternating; the two calls draw their own inference noise, so '
                         'mse_max_abs_diff is between two draws, not a parity figure; large512: the kernel alone, fused against the tiled render '
                         'followed by a torch sum',
                  shapes=shapes)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps({k: {r: round(v['ms'], 3) for r, v in s['rows'].items()} for k, s in shapes.items()}))


if __name__ == '__main__':
    main()
