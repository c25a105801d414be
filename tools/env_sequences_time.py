#!/usr/bin/env python
"""Time whole-sequence data synthesis (stove_amd/envs/synth.py, csrc/env_sequences.hip) at the reference's shape: B sequences of T = 100
steps of the four presets at res 32, gravity and multibilliards also at the reference's stock res 50.

    python tools/env_sequences_time.py [--sequences 1000 --steps 100 --host-sequences 64 --workers 16 --repeats 7
                                        --out profiles/env_sequences.json]

Per configuration:
  launch_ms          the one stove_env_sequences launch on B sequences (device events around it): median and range of `repeats`
                     launches after one warm-up launch.  Its starts are the `host-sequences` drawn ones, tiled to B rows
  draw_starts_ms     draw_starts alone, per sequence: the per-sequence Python that remains (constructors' rejection sampling and, for
                     avoidance, the action policy's rng.choice).  Reported separately, not folded into the launch's figure
  numpy_ms           the numpy specification (BatchedSequences.run) on the host-sequences starts, per sequence
  parallel_ms        envs.synth_sequences_parallel with `workers` forked workers on host-sequences sequences, per sequence: how the
                     sequences were made before, and the figure to compare against.  It forks, so it runs first, before the process
                     touches the GPU
The committed profiles/env_sequences.json also carries `forms_ms`: the kernel's alternating form (step, barrier, paint, barrier) and
gravity's force loop on one lane, timed against the kept form from a scratch build at the same shape; those forms are not
in the tree, so this tool cannot time them again.
The host figures are per sequence because they are linear in the sequence count; B x the figure is the cost of B.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [('billiards', None), ('multibilliards', None), ('avoidance', None), ('gravity', None), ('gravity', 50), ('multibilliards', 50)]


def _timed(call, repeats):
    """device events around `call`, `repeats` times -> dict(median, min, max, launches) in ms"""
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    times.sort()
    return dict(median=times[len(times) // 2], min=times[0], max=times[-1], launches=len(times))


def counter_rows(args):
    """--starts counter: per configuration the counter-based stream's row, written under configs[key]['counter'] of the profile (the
    host rows already there are kept; none is measured again):
      draw_launch_ms       the one stove_env_draw_starts launch on B sequences of seeds 0 .. B - 1, as launch_ms above
      both_launches_ms     that launch and the stove_env_sequences launch on its outputs, device events around the pair
      numpy_draw_ms_per_sequence   draw_starts_counter, the numpy specification, on host-sequences sequences
    The launch's outputs are checked bit for bit against the specification on the first host-sequences sequences in the same run."""
    from stove_amd import build, ops
    from stove_amd.envs import synth
    build.build_library()
    if not torch.cuda.is_available():
        raise SystemExit('env_sequences_time.py measures on a GPU; none found')
    B, T, H = args.sequences, args.steps, args.host_sequences
    dev = torch.device('cuda:0')
    doc = dict(sequences=B, steps=T, host_sequences=H, workers=args.workers, device=torch.cuda.get_device_name(0), configs={})
    if os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    for preset, res in CONFIGS:
        key = '%s_res%d' % (preset, res or 32)
        t0 = time.perf_counter()
        spec = synth.draw_starts_counter(preset, H, T, res=res)
        numpy_ms = 1e3 * (time.perf_counter() - t0) / H
        acting = spec['actions'] is not None
        s, r1, m1, factor = synth._preset_settings(preset, acting, res)
        r = torch.from_numpy(r1).to(dev).repeat(B, 1)
        m = torch.from_numpy(m1).to(dev).repeat(B, 1)
        draw = lambda out=None: ops.env_draw_starts(r, T, 0, s['hw'], gravity=s['gravity'], v_factor=factor or 0.0, with_actions=acting, out=out)
        run = lambda d, out=None: ops.env_sequences(d['x0'], d['v0'], r, m, d['actions'], T, s['granularity'], s['res'], s['hw'], s['t'],
                                                    s['friction'], s['action_force'], use_colors=s['use_colors'], drift=s['drift'],
                                                    gravity=s['gravity'], out=out)
        d = draw()          # the warm-up launches; the timed ones write into the same tensors
        out = run(d)
        torch.cuda.synchronize()
        same = all(np.array_equal(d[k][:H].cpu().numpy(), spec[k]) for k in ('x0', 'v0', 'tries', 'status') + (('actions',) if acting else ()))
        if not acting:
            del d['actions']
        row = dict(draw_launch_ms=_timed(lambda: draw(d), args.repeats), both_launches_ms=_timed(lambda: run(draw(d), out), args.repeats),
                   starts_equal_numpy_bitwise=bool(same), numpy_draw_ms_per_sequence=numpy_ms, sequences=B,
                   tries_mean=float(d['tries'].double().mean()), tries_max=int(d['tries'].max()), without_start=int((d['status'] != 0).sum()))
        row['draw_launch_ms_per_sequence'] = row['draw_launch_ms']['median'] / B
        row['both_launches_ms_per_sequence'] = row['both_launches_ms']['median'] / B
        doc['configs'].setdefault(key, {})['counter'] = row
        print(key, json.dumps(row), flush=True)
        del out, d
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    print('wrote', args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sequences', type=int, default=1000)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--host-sequences', type=int, default=64)
    ap.add_argument('--workers', type=int, default=16)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'env_sequences.json'))
    ap.add_argument('--starts', choices=('host', 'counter'), default='host', help='counter: time the counter-based stream, starts and '
                    'actions drawn on the device (stove_env_draw_starts), and add its row to every configuration of --out')
    args = ap.parse_args()
    if args.starts == 'counter':
        return counter_rows(args)
    from stove_amd import build
    from stove_amd.envs import envs, synth
    build.build_library()
    B, T, H = args.sequences, args.steps, args.host_sequences
    host = {}
    for preset, res in CONFIGS:          # everything that forks or runs on the host first
        key = '%s_res%d' % (preset, res or 32)
        t0 = time.perf_counter()
        envs.synth_sequences_parallel(preset, H, T, res=res, workers=args.workers)
        t1 = time.perf_counter()
        starts = synth.draw_starts(preset, H, T, res=res)
        t2 = time.perf_counter()
        spec = synth.BatchedSequences(starts).run(T)
        t3 = time.perf_counter()
        host[key] = dict(starts=starts, spec=spec, parallel_ms=1e3 * (t1 - t0) / H, draw_starts_ms=1e3 * (t2 - t1) / H,
                         numpy_ms=1e3 * (t3 - t2) / H)
        print(key, {k: round(v, 3) for k, v in host[key].items() if k.endswith('_ms')}, flush=True)
    if not torch.cuda.is_available():
        raise SystemExit('env_sequences_time.py measures on a GPU; none found')
    from stove_amd import ops
    dev = torch.device('cuda:0')
    results = {}
    for preset, res in CONFIGS:
        key = '%s_res%d' % (preset, res or 32)
        h = host[key]
        st, s = h['starts'], h['starts']['settings']
        rows = np.arange(B) % H
        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a[rows])).to(dev)
        x0, v0, r, m, acts = (up(st[k]) for k in ('x0', 'v0', 'r', 'm', 'actions'))
        call = lambda out=None: ops.env_sequences(x0, v0, r, m, acts, T, s['granularity'], s['res'], s['hw'], s['t'], s['friction'],
                                                  s['action_force'], use_colors=s['use_colors'], drift=s['drift'], gravity=s['gravity'], out=out)
        out = call()          # the warm-up launch; the timed ones write into the same tensors
        torch.cuda.synchronize()
        same = bool(np.array_equal(out['y'][:H].cpu().numpy().view(np.int64), h['spec']['y'].view(np.int64)))
        times = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call(out)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        times.sort()
        results[key] = dict(launch_ms=dict(median=times[len(times) // 2], min=times[0], max=times[-1], launches=len(times)),
                            launch_ms_per_sequence=times[len(times) // 2] / B, states_equal_numpy_bitwise=same,
                            draw_starts_ms_per_sequence=h['draw_starts_ms'], numpy_ms_per_sequence=h['numpy_ms'],
                            parallel_ms_per_sequence=h['parallel_ms'])
        print(key, json.dumps(results[key]), flush=True)
        del out
    doc = dict(sequences=B, steps=T, host_sequences=H, workers=args.workers, device=torch.cuda.get_device_name(0), configs=results)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
