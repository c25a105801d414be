"""Float64 restatement of the state-supervised baseline (reference model/supairvised/dynamics.py:39-107 with debug_rollout = True,
train.py:77-108), composed from the oracle's core step.  tests/golden/g31_supervised_f64.npz holds what the reference's own module
gives (tools/make_sup_goldens.py); tests/test_sup_cpu.py holds this file to it."""
import torch

import stove_oracle as O
from analytic_weights import analytic_tensor, fan_ins

SUP_REGIMES = ('init', 'half', 'analytic')          # 'analytic': one-step cases only (chaotic under this recursion)


def sup_config(cl, nonlinear='relu', **kw):
    return O.default_config(cl=cl, debug_nonlinear=nonlinear, **kw)


def core0_shapes(cl):
    """{reference state-dict name: shape} of what the supervised model differentiates: the (cl, cl) encoder and core 0 (28 tensors)"""
    lin = {'dyn.state_enc': (cl, cl)}
    for name, dims in (('self_cores', [(cl, cl), (cl, cl)]), ('rel_cores', [(1 + 2 * cl, 2 * cl), (2 * cl, cl), (cl, cl)]),
                       ('att_net', [(1 + 2 * cl, 2 * cl), (2 * cl, cl), (cl, 1)]), ('affector', [(cl, cl)] * 3),
                       ('out', [(2 * cl, cl), (cl, cl)])):
        for k, (i, o) in enumerate(dims):
            lin['dyn.%s.0.%d' % (name, k)] = (i, o)
    shapes = {}
    for k, (i, o) in lin.items():
        shapes[k + '.weight'] = (o, i)
        shapes[k + '.bias'] = (o,)
    return shapes


def regime_tensor(name, shape, regime, dtype=torch.float64, fan_in=None):
    """'init' / 'analytic' of analytic_weights; 'half': 'analytic' with every weight matrix halved, biases untouched"""
    if regime == 'half':
        t = analytic_tensor(name, shape, torch.float64, 'analytic', fan_in)
        return (t * 0.5 if name.endswith('.weight') else t).to(dtype)
    return analytic_tensor(name, shape, torch.float64, regime, fan_in).to(dtype)


def sup_params(cl, regime, dtype=torch.float64):
    shapes = core0_shapes(cl)
    fi = fan_ins(shapes)
    return {k: regime_tensor(k, shp, regime, dtype, fi.get(k)).requires_grad_() for k, shp in shapes.items()}


def sup_rollout_ref(c, params, x, latent0, R, with_codes=False):
    """x (B,V,N,4), latent0 (B,N,cl-4) -> pred (B,R,N,4) [, codes (B,V-1+R,N,cl): every step's input]"""
    core = lambda code: O.dynamics_forward(c, params, code, lim_enc=4)[0]          # noqa: E731
    code = torch.cat([x[:, 0], latent0], -1)
    codes = []
    for i in range(1, x.shape[1]):
        codes.append(code)
        code = torch.cat([x[:, i], core(code)[..., 4:]], -1)
    preds = []
    for _ in range(R):
        codes.append(code)
        res = core(code)
        code = torch.cat([res[..., :2] + code[..., :2], res[..., 2:]], -1)
        preds.append(code[..., :4])
    pred = torch.stack(preds, 1)
    return (pred, torch.stack(codes, 1)) if with_codes else pred


def sup_loss_ref(pred, future, discount, end=4, with_delta=True):
    """-> (total, pred_loss, delta_loss); the reconstruction term of the reference is mse(x, x) = 0"""
    mse = lambda a, b: ((a - b) ** 2).mean()          # noqa: E731
    R = pred.shape[1]
    pred_loss = sum(discount ** (t + 1) * mse(pred[:, t, :, :end], future[:, t, :, :end]) for t in range(R))
    delta_loss = pred.new_zeros(())
    if with_delta:
        dp, df = pred[:, 1:] - pred[:, :-1], future[:, 1:] - future[:, :-1]
        for t in range(R - 1):
            delta_loss = delta_loss + discount ** (t + 1) * 6 * mse(dp[:, t, :, :end], df[:, t, :, :end])
    return pred_loss + delta_loss, pred_loss, delta_loss
