"""Time Stove.rollout(sample=True) both ways it can run -> profiles/rollout_sample.json.

B = 256, N = 3, num = 92 (the shape README quotes for the mean rollout), cl = 32, no noise_fn (the library's generator draws):

  fused      under torch.no_grad: one draw of B num N 16 normals + one launch of the sampling rollout kernel
  step_loop  the same call with autograd enabled on a model whose parameters do not require grad: the host loop of single
             differentiable steps (Dynamics.forward, constrain_z_dyn, randn, log-prob per step) -- what every sampling rollout ran
             before the fused path existed
  mean       Stove.rollout(sample=False), the one-launch mean prediction, as the neighbour the fused path is expected to sit next to

Events on the current stream around one call, 5 warm-up calls each, median of 21; the three are timed in alternation (one repetition
of each per round), so that whatever else the machine is doing falls on all of them alike; min and max are kept as the spread.

    python tools/rollout_sample_time.py [--out profiles/rollout_sample.json] [--parity PARITY_ERRORS_JSON]

--parity: a parity record of the -m gpu run (tests/conftest.py writes it); its rollout_sample.* entries are copied into the output.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                                                  # noqa: E402


def time_alternating(fns, warm=5, reps=21):
    """{name: callable} -> {name: [ms, ...]}: `reps` rounds, every callable once per round"""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rollout_sample.json'))
    ap.add_argument('--parity', default=None)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--objects', type=int, default=3)
    ap.add_argument('--steps', type=int, default=92)
    args = ap.parse_args()
    from stove_amd import build
    build.build_library()
    from stove_amd.video_prediction.config import StoveConfig
    from stove_amd.video_prediction.stove import Stove
    dev = torch.device('cuda:0')
    cfg = StoveConfig()
    cfg.num_obj, cfg.width, cfg.height = args.objects, 32, 32
    cfg.device, cfg.dtype, cfg.random_seed = dev, torch.float32, 42
    cfg.action_conditioned, cfg.action_space = False, None
    if args.objects != 3:
        cfg.debug_match_objects = 'greedy'
    torch.manual_seed(0)
    st = Stove(cfg).to(dev)
    for p in st.parameters():
        p.requires_grad_(False)
    B, N, num = args.batch, args.objects, args.steps
    z_last = torch.cat([torch.rand(B, N, 2, device=dev) * 0.2 + 0.1, torch.rand(B, N, 16, device=dev) - 0.5], -1)

    def fused():
        with torch.no_grad():
            return st.rollout(z_last, num=num, sample=True)

    def step_loop():
        with torch.enable_grad():
            return st.rollout(z_last, num=num, sample=True)

    def mean():
        with torch.no_grad():
            return st.rollout(z_last, num=num)
    zf, lq, _ = fused()
    zl, ll, _ = step_loop()
    assert zf.shape == zl.shape == (B, num, N, 18) and lq.shape == ll.shape == (B, num, N, 16)
    assert bool(torch.isfinite(zf).all()) and bool(torch.isfinite(lq).all())
    times = time_alternating({'fused': fused, 'step_loop': step_loop, 'mean': mean})
    rows = {}
    for k, v in times.items():
        med = statistics.median(v)
        rows[k] = dict(ms=med, us_per_step=1e3 * med / num, min_ms=min(v), max_ms=max(v))
        print(k, rows[k], flush=True)
    result = dict(device=torch.cuda.get_device_name(0), B=B, N=N, num=num, cl=32,
                  method='hip events around one Stove.rollout call, 5 warm-up calls, median of 21, the three variants alternating; '
                         'fused = no_grad (one noise draw + one kernel), step_loop = autograd enabled on frozen parameters (host loop '
                         'of single steps), mean = sample=False',
                  rows=rows, speedup_fused_over_step_loop=rows['step_loop']['ms'] / rows['fused']['ms'])
    if args.parity:
        with open(args.parity) as fh:
            result['parity'] = {k: v for k, v in json.load(fh).items() if k.startswith('rollout_sample.')}
    with open(args.out, 'w') as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps({k: result[k] for k in ('rows', 'speedup_fused_over_step_loop')}))


if __name__ == '__main__':
    main()
