#!/usr/bin/env python
"""Write tests/golden/g22_pixel_error_f64.npz: the reference's Supair.reconstruct_from_z (model/video_prediction/supair.py of a
reference checkout) and the two lines of its scripts/pixel_error.py that turn rendered frames into the per-step pixel error, in
float64, so that tests/render_ref.py and the HIP render can be held against them without the reference.

    python tools/make_pixel_goldens.py --reference /path/to/reference

Two single-channel cases, frames of 32 x 32 and 50 x 50 pixels with 10 x 10 glimpses: 2 sequences x 6 frames x 3 objects, weights from
the analytic fill of tests/golden/analytic_weights.py (not stored).  Per case (keys suffixed _r32 / _r50): x (n, T, 1, w, h) frames,
z (n, T, 3, 4) states with objects over the frame's edges, an overlapping pair and tiny boxes among them, bg_max / obj_max (the SPNs'
max-activation images), mpe_patches = spn_mpe(z[:, 0], x[:, 0]) (n, 3, 100), recon_max = reconstruct_from_z(z), recon_mpe_single = reconstruct_from_z(z, x[:, 0], max_activation=False,
single_image=True), and mse (T,): the reference's own clamp-and-mean statements (run from its file) on (x, recon_max)."""
import argparse
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SEQ, T_LEN, N_OBJ = 2, 6, 3
SIZES = (32, 50)


def load_reference(path):
    """the reference's Supair class; third-party modules it imports and this machine lacks become empty stand-ins"""
    import scipy
    for name in ('spriteworld', 'spriteworld.renderers', 'spriteworld.sprite', 'imageio', 'setproctitle'):
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    if not hasattr(sys.modules['spriteworld.sprite'], 'Sprite'):
        sys.modules['spriteworld.sprite'].Sprite = object
        sys.modules['spriteworld'].renderers = sys.modules['spriteworld.renderers']
    if not hasattr(sys.modules['setproctitle'], 'setproctitle'):
        sys.modules['setproctitle'].setproctitle = lambda *_: None
    if not hasattr(scipy, 'rand'):                    # (the reference's region graphs draw with names scipy has dropped)
        scipy.rand, scipy.randn = np.random.rand, np.random.randn
    for name in [m for m in sys.modules if m == 'model' or m.startswith('model.')]:
        del sys.modules[name]                         # `model` must resolve to the reference's package, not to this tree's
    sys.path.insert(0, path)
    from model.video_prediction.config import StoveConfig
    from model.video_prediction.supair import Supair
    return StoveConfig, Supair


def load_mse_lines(path):
    """the two statements of the reference's scripts/pixel_error.py that turn (true_images, model_images) into `mse`, compiled from that
    file as it stands -> f(namespace) -> mse"""
    with open(os.path.join(path, 'scripts', 'pixel_error.py')) as f:
        lines = [ln.strip() for ln in f]
    picked = [ln for ln in lines if ln.startswith('model_images = torch.clamp(') or ln.startswith('mse = torch.mean(')]
    if len(picked) != 2:
        raise RuntimeError('scripts/pixel_error.py: expected the clamp and the mean statements, found %r' % picked)
    code = compile('\n'.join(picked), os.path.join(path, 'scripts', 'pixel_error.py'), 'exec')

    def run(ns):
        exec(code, ns)
        return ns['mse']
    return run


def draw_z(g):
    z = torch.zeros(N_SEQ * T_LEN, N_OBJ, 4, dtype=torch.float64)
    z[..., 0] = 0.1 + 0.5 * torch.rand(N_SEQ * T_LEN, N_OBJ, generator=g, dtype=torch.float64)
    z[..., 1] = z[..., 0] * (0.75 + 0.5 * torch.rand(N_SEQ * T_LEN, N_OBJ, generator=g, dtype=torch.float64))
    z[..., 2:] = 2.2 * torch.rand(N_SEQ * T_LEN, N_OBJ, 2, generator=g, dtype=torch.float64) - 1.1
    z[0, 1, 2:] = z[0, 0, 2:] + 0.05                  # an overlapping pair
    z[1, 0, 2:] = torch.tensor([0.95, -0.97])         # partly out of the frame
    z[2, :, 0], z[2, :, 1] = 0.1, 0.075               # tiny boxes
    z[3, :, 2:] = z[3, 0:1, 2:]                       # all objects stacked
    return z.view(N_SEQ, T_LEN, N_OBJ, 4)


def case(StoveConfig, Supair, fill, mse_lines, res):
    torch.set_default_dtype(torch.float64)
    c = StoveConfig()
    c.num_obj, c.width, c.height = N_OBJ, res, res
    c.device, c.dtype, c.random_seed = torch.device('cpu'), torch.float64, 42
    c.action_conditioned, c.action_space, c.skip = False, None, 2
    c.r, c.coord_lim, c.num_frames = 1.2, 10, 100
    sup = Supair(c)
    fill(sup)
    g = torch.Generator().manual_seed(2200 + res)
    x = (torch.rand(N_SEQ, T_LEN, 1, res, res, generator=g, dtype=torch.float64) ** 3).float().double()     # float32-representable
    z = draw_z(g)
    with torch.no_grad():
        recon_max = sup.reconstruct_from_z(z)
        recon_single = sup.reconstruct_from_z(z, x[:, 0], max_activation=False, single_image=True)
        mse = mse_lines({'torch': torch, 'true_images': x, 'model_images': recon_max})
        out = dict(x=x, z=z, bg_max=sup.spn_max_activation(sup.bg_spn), obj_max=sup.spn_max_activation(sup.obj_spn),
                   recon_max=recon_max, recon_mpe_single=recon_single, mse=mse, mpe_patches=sup.spn_mpe(z[:, 0], x[:, 0]))
    return {'%s_r%d' % (k, res): v.detach().cpu().numpy().astype(np.float64) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of a reference checkout (holds model/video_prediction/supair.py)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'g22_pixel_error_f64.npz'))
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    from analytic_weights import analytic_tensor, fan_ins
    StoveConfig, Supair = load_reference(args.reference)
    mse_lines = load_mse_lines(args.reference)

    def fill(sup):
        with torch.no_grad():
            named = {'sup.' + name: p for name, p in sup.named_parameters()}
            fi = fan_ins({k: tuple(p.shape) for k, p in named.items()})
            for name, p in named.items():
                p.copy_(analytic_tensor(name, p.shape, p.dtype, 'analytic', fi.get(name)))

    out = {'sizes': np.array(SIZES, dtype=np.int64)}
    for res in SIZES:
        out.update(case(StoveConfig, Supair, fill, mse_lines, res))
        print('res %d: mse %s' % (res, np.array2string(out['mse_r%d' % res], precision=6)))
    np.savez_compressed(args.out, **out)
    print('wrote', args.out, os.path.getsize(args.out), 'bytes')


if __name__ == '__main__':
    main()
