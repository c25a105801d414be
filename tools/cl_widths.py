"""Time the dynamics kernels per dependent step at state-code lengths 16 / 32 / 64 -> profiles/cl_widths.json.

Two groups of rows, B = 256, N = 3 and 6, event-timed on the current stream, 3 warm-up runs, median of 11:

  recursion  one ops.dyn_loop call over T = 100 frames (Ts = 98 dependent steps) and its backward, us per step = time / Ts.  The
             parameter image is built once outside the timed region; the backward is timed between events of its own, as one
             torch.autograd.grad call on a graph built beforehand (retain_graph) with pre-built upstream gradients -- the recursion's
             backward launch(es) and nothing else.  cl = 32 dispatches to the small-graph kernels (gnn_small*.hip) at these N.
  step       one ops.gnn_step call (a single GNN step, B = 256) and its backward.  At cl = 32 this is the MFMA formulation of gnn.hip
             that the N > 6 path uses, run at N = 3 / 6: the like-for-like neighbour of the width-generic kernels.

    python tools/cl_widths.py [--out profiles/cl_widths.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                                                  # noqa: E402


def time_ms(fn, warm=3, reps=11):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cl_widths.json'))
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--frames', type=int, default=100, help='T; the recursion runs T - 2 dependent steps')
    args = ap.parse_args()
    from stove_amd import build, ops
    build.build_library()
    from stove_amd.video_prediction.config import StoveConfig
    from stove_amd.video_prediction.dynamics import Dynamics
    dev = torch.device('cuda:0')
    B, Ts = args.batch, args.frames - 2
    rows = []
    for cl in (16, 32, 64):
        for N in (3, 6):
            cfg = StoveConfig()
            cfg.num_obj, cfg.device, cfg.dtype, cfg.cl = N, dev, torch.float32, cl
            cfg.action_conditioned, cfg.action_space = False, None
            cfg.transition_lik_std = [0.01] * (cl // 2)
            torch.manual_seed(0)
            dyn = Dynamics(cfg).to(dev)
            D = cl // 2
            image = tuple(t.detach().requires_grad_() for t in dyn.param_image(0))      # built once, a leaf of its own
            z1 = (torch.rand(B, N, D + 2, device=dev) - 0.5).requires_grad_()
            zsup = torch.rand(B, Ts, N, 6, device=dev) - 0.5
            zsstd = torch.rand(B, Ts, N, 6, device=dev) * 0.1 + 0.05
            eps = torch.randn(B, Ts, N, D + 2, device=dev)

            def loop():
                return ops.dyn_loop(z1, zsup, zsstd, eps, None, image, 2, dyn.use_elu, dyn.loop_consts())
            f = time_ms(loop)
            z, zdyn, _, mean, std, _ = loop()
            outs = (z, zdyn, mean, std)
            ups = tuple(torch.ones_like(t) for t in outs)
            b = time_ms(lambda: torch.autograd.grad(outs, (z1, image[0], image[1]), ups, retain_graph=True))
            rows.append(dict(kind='recursion', cl=cl, N=N, B=B, T=args.frames, Ts=Ts, fwd_us_per_step=1e3 * f / Ts,
                             bwd_us_per_step=1e3 * b / Ts, fwd_ms=f, bwd_ms=b))
            print(rows[-1], flush=True)

            s_in = (torch.rand(B, N, D, device=dev) - 0.5).requires_grad_()

            def step():
                return ops.gnn_step(s_in, image, 2, dyn.use_elu, None, cl=cl)
            f = time_ms(step)
            res, pred = step()
            up = torch.ones_like(res)
            b = time_ms(lambda: torch.autograd.grad((res,), (s_in, image[0], image[1]), (up,), retain_graph=True))
            rows.append(dict(kind='step', cl=cl, N=N, B=B, fwd_us=1e3 * f, bwd_us=1e3 * b))
            print(rows[-1], flush=True)
    with open(args.out, 'w') as fh:
        json.dump(dict(device=torch.cuda.get_device_name(0),
                       method='hip events around the call, 3 warm-up runs, median of 11; parameter image built outside the timed region; '
                              'backward = one torch.autograd.grad on a retained graph',
                       rows=rows), fh, indent=1)


if __name__ == '__main__':
    main()
