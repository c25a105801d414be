"""The state-supervised dynamics model (reference model/supairvised/dynamics.py:14-107): the interaction network of `Dynamics` on
ground-truth object states (x, y, vx, vy), rolled out with the whole cl-wide result fed back.

Only the reference's working configuration is built: debug_rollout = True (its other branch feeds 4-wide labels to the 16-input
encoder and raises), not action-conditioned and without appearance features (a supervised code is already cl wide, and a core input
can be at most cl wide: the kernels' encoder image is [cl][cl]).
"""
import torch

from .. import ops
from ..video_prediction.dynamics import Dynamics


class SupervisedDynamics(Dynamics):
    SUPPORTED_CL = (16, 64)          # the width-generic kernels (csrc/gnn_cl.hip, gnn_sup.hip)

    def __init__(self, config):
        if config.action_conditioned or config.debug_core_appearance:
            raise NotImplementedError(
                'the supervised baseline is built for data without actions and without debug_core_appearance: its state code fills '
                'the cl-wide core input, so an action embedding (+4) or appearances (+%d) do not fit the [cl][cl] encoder'
                % config.debug_appearance_dim)
        super().__init__(config, enc_input_size=config.cl)          # (the reference's 16 at its cl = 16)

    def _init_transition_std(self):
        pass                         # no transition likelihood in this model

    def step(self, code):
        """One core step on a cl-wide code, lim_enc = 4: positions and velocities reach the edge layers raw."""
        return super().forward(code, 0, lim_enc=4)[0]

    def forward(self, x, num_rollout=8, debug_rollout=True, actions=None, fused=None, latent=None, return_codes=False):
        """x (n, V, o, 4) observed states -> (predicted states (n, num_rollout, o, 4), x).

        latent: (n, o, cl - 4) initial latent instead of a standard-normal draw.  fused: the one-launch kernels (ops.sup_rollout)
        or, False, the loop of core steps under autograd that specifies them; None: see FUSED_DEFAULT.  return_codes: also the input
        code of every step, (n, V - 1 + num_rollout, o, cl)."""
        if not debug_rollout:
            raise ValueError('SupervisedDynamics runs with debug_rollout=True only: the reference\'s other branch applies the '
                             'cl-input state encoder to the 4-wide labels and fails (supairvised/dynamics.py:87)')
        if actions is not None:
            raise NotImplementedError('the supervised baseline is not action-conditioned (its state code fills the core input)')
        n, V, o = x.shape[:3]
        cl = self.c.cl
        if latent is None:
            latent = torch.randn(n, o, cl - 4, dtype=x.dtype, device=x.device)
        on_gpu = x.is_cuda and x.dtype == torch.float32
        if fused is None:
            fused = on_gpu and FUSED_DEFAULT
        if fused:
            if not on_gpu:
                raise RuntimeError('the fused supervised rollout runs on float32 CUDA tensors only')
            image, sink = self.kernel_params(0)
            out = ops.sup_rollout(x, latent, image, num_rollout, self.use_elu, sink, want_codes=return_codes)
            return (out[0], x, out[1]) if return_codes else (out, x)
        code = torch.cat([x[:, 0], latent], -1)
        codes = []
        for i in range(1, V):
            codes.append(code)
            code = torch.cat([x[:, i], self.step(code)[..., 4:]], -1)        # observed states go into the code as they are
        preds = []
        for _ in range(num_rollout):
            codes.append(code)
            res = self.step(code)
            code = torch.cat([res[..., :2] + code[..., :2], res[..., 2:]], -1)
            preds.append(code[..., :4])
        pred = torch.stack(preds, 1)
        return (pred, x, torch.stack(codes, 1)) if return_codes else (pred, x)


# What fused=None resolves to on float32 CUDA tensors.  tools/sup_time.py measured the one-launch path against the composed loop at the
# reference's training shape (B = 256, V = 6, R = 8, N = 3, cl = 16): 0.54 ms against 1.89 ms per training step on an MI355X
# (profiles/sup_rollout.json records the numbers and the decision).
FUSED_DEFAULT = True
