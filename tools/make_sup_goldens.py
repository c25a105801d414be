#!/usr/bin/env python
"""Write tests/golden/g31_supervised_f64.npz: the reference's state-supervised baseline in float64 -- SupervisedDynamics
(model/supairvised/dynamics.py, debug_rollout=True) at cl = 16, SupTrainer.compute_loss (model/supairvised/train.py) and
StoveDataset with supairvised = True (model/video_prediction/load_data.py) -- so that tests/sup_ref.py and the dataset can be held
to them without the reference.

    python tools/make_sup_goldens.py --reference /path/to/reference

Cases (keys prefixed n{N}B{B}V{V}R{R}_{fill}_{nonlinear}/): (N, B, V, R) = (3, 4, 3, 4) and (2, 2, 1, 1) -- B, N >= 2, the reference
squeezes its latent draw -- under the 'init' and 'half' fills of tests/sup_ref.py (weights are not stored) and both nonlinearities.
Per case: x, latent0 (fed through a stand-in for the module's latent_prior), future, pred, losses (total, pred, recon) and
grad/<name>: the gradient of total in every parameter that has one.  Dataset: 2 episodes x 20 frames x 3 objects at 8 x 8 pixels ->
ds_y, ds_X (the inputs), ds_total_data, ds_total_img and the sample ds[3]."""
import argparse
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tests', 'golden')):
    sys.path.insert(0, p)
import sup_ref as S          # noqa: E402

SHAPES = ((3, 4, 3, 4), (2, 2, 1, 1))


def load_reference(path):
    """the reference's classes; third-party modules it imports and this machine lacks become empty stand-ins"""
    for name in ('imageio', 'matplotlib', 'matplotlib.pyplot', 'matplotlib.animation', 'matplotlib.patches', 'matplotlib.gridspec',
                 'visdom', 'setproctitle', 'pandas'):
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    for name in [m for m in sys.modules if m == 'model' or m.startswith('model.')]:
        del sys.modules[name]                         # `model` must resolve to the reference's package, not to this tree's
    sys.path.insert(0, path)
    from model.supairvised.config import SupStoveConfig
    from model.supairvised.dynamics import SupervisedDynamics
    from model.supairvised.train import SupTrainer
    from model.video_prediction.load_data import StoveDataset
    return SupStoveConfig, SupervisedDynamics, SupTrainer, StoveDataset


class FedLatent:
    """stands in for the module's latent_prior: rsample(shape) returns the recorded latent with the trailing axis the reference squeezes"""

    def __init__(self, latent):
        self.latent = latent

    def rsample(self, shape):
        assert tuple(shape) == tuple(self.latent.shape), (shape, self.latent.shape)
        return self.latent.unsqueeze(-1)


def config(SupStoveConfig, n_obj, nonlinear, R):
    c = SupStoveConfig()
    c.num_obj, c.num_rollout, c.debug_nonlinear = n_obj, R, nonlinear
    c.device, c.dtype = torch.device('cpu'), torch.float64
    c.action_conditioned, c.action_space = False, None
    return c


def case(ref, shape, fill, nonlinear, seed):
    SupStoveConfig, SupervisedDynamics, SupTrainer, _ = ref
    N, B, V, R = shape
    c = config(SupStoveConfig, N, nonlinear, R)
    dyn = SupervisedDynamics(c).double()
    shapes = S.core0_shapes(c.cl)
    fi = S.fan_ins(shapes)
    with torch.no_grad():
        for name, p in dyn.named_parameters():
            key = 'dyn.' + name
            if key in shapes:
                assert tuple(p.shape) == tuple(shapes[key]), key
                p.copy_(S.regime_tensor(key, p.shape, fill, torch.float64, fi.get(key)))
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)          # noqa: E731
    states = lambda T: torch.cat([2.0 * r(B, T, N, 2), 0.8 * r(B, T, N, 2) - 0.4], -1)          # noqa: E731
    x, future = states(V), states(R)
    latent0 = torch.randn(B, N, c.cl - 4, generator=g, dtype=torch.float64)
    dyn.latent_prior = FedLatent(latent0)
    pred, recon = dyn(x, num_rollout=R, debug_rollout=True)
    stub = types.SimpleNamespace(c=c)
    total, pred_loss, recon_loss = SupTrainer.compute_loss(stub, x, future, recon, pred)
    total.backward()
    out = {'x': x, 'latent0': latent0, 'future': future, 'pred': pred.detach(),
           'losses': torch.stack([total.detach(), pred_loss.detach(), recon_loss.detach()])}
    for name, p in dyn.named_parameters():
        if p.grad is not None:
            out['grad/dyn.' + name] = p.grad
    return {k: v.numpy() for k, v in out.items()}


def dataset(ref):
    SupStoveConfig, _, _, StoveDataset = ref
    c = config(SupStoveConfig, 3, 'relu', 4)
    c.num_visible, c.num_episodes = 3, 1000
    rs = np.random.RandomState(31)
    y = np.concatenate([10.0 * rs.rand(2, 20, 3, 2), 2.0 * rs.rand(2, 20, 3, 2) - 1.0], -1)
    X = rs.rand(2, 20, 8, 8, 3) * (rs.rand(2, 20, 8, 8, 3) < 0.5)
    ds = StoveDataset(c, data={'X': X.copy(), 'y': y.copy()})
    out = {'ds_y': y, 'ds_X': X, 'ds_total_data': np.asarray(ds.total_data), 'ds_total_img': np.asarray(ds.total_img)}
    for k, v in ds[3].items():
        out['ds_sample/' + k] = np.asarray(v)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True)
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'g31_supervised_f64.npz'))
    args = ap.parse_args()
    torch.set_default_dtype(torch.float64)
    ref = load_reference(args.reference)
    out, seed = {}, 3100
    for shape in SHAPES:
        for fill in ('init', 'half'):
            for nonlinear in ('relu', 'leaky_relu'):
                seed += 1
                key = 'n%dB%dV%dR%d_%s_%s/' % (*shape, fill, nonlinear)
                for k, v in case(ref, shape, fill, nonlinear, seed).items():
                    out[key + k] = v
    out.update(dataset(ref))
    np.savez_compressed(args.out, **out)
    print(args.out, os.path.getsize(args.out), 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
    main()
