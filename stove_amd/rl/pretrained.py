"""Start states for the model-based PPO arm (counterpart of `load_and_encode` in the reference's model/rl/main_rl.py:137-161): every
window of `window` frames of recorded action-conditioned sequences goes through the model once, and the last inferred state and
object appearances of the window become one start state.  Objects are reordered so that the one with the largest first appearance
channel -- the red, controlled ball -- comes first and the others keep their order, which is the order the policy was built for.

All windows of all sequences are batched through the model in chunks; the reference walks the windows one `Stove` forward at a time.
The result depends only on the data and the model, so it is computed once per run: the reference recomputes it for every batch, which
is an accident of its training loop (the call sits inside it) and is not reproduced."""
import pickle

import torch


def red_first(states, appearances):
    """states (K, N, D), appearances (K, N, C) -> both with the object of the largest appearances[:, :, 0] moved to the front (the
    first such object on a tie, as argmax takes it) and the other objects in their order"""
    K, N = appearances.shape[:2]
    red = torch.argmax(appearances[:, :, 0], dim=1)
    rest = torch.arange(N, device=red.device).expand(K, N)
    rest = rest[rest != red[:, None]].reshape(K, N - 1)
    order = torch.cat([red[:, None], rest], 1)
    take = lambda t: torch.gather(t, 1, order[:, :, None].expand(-1, -1, t.shape[2]))
    return take(states), take(appearances)


@torch.no_grad()
def load_and_encode(path_or_arrays, state_model, device, window=8, chunk=256):
    """path_or_arrays: a pickle of, or itself, a dict with 'X' frames in [0, 1], (n, T, res, res, 3) or (n, T, 3, res, res), and 'action'
    (n, T, actions) one-hot rows -> (encoded states (n (T - window), N, 18), appearances (n (T - window), N, app_dim)) float32 on
    `device`, sequence-major as the reference flattens them.  Frames reach the model as StoveDataset feeds them in training,
    channel-last data through transpose (0, 1, 4, 2, 3); the reference's permute(0, 1, 4, 3, 2) at this place also swaps the two
    image axes against its own training data, which is not reproduced."""
    data = path_or_arrays
    if not isinstance(data, dict):
        with open(data, 'rb') as fh:
            data = pickle.load(fh)
    X = torch.as_tensor(data['X']).float()
    if X.dim() != 5:
        raise ValueError("data['X'] must hold (n, T, res, res, 3) or (n, T, 3, res, res) frames, not %s" % (tuple(X.shape),))
    if X.shape[-1] == 3:
        X = X.permute(0, 1, 4, 2, 3)
    actions = torch.as_tensor(data['action']).float()
    n, T = X.shape[:2]
    steps = T - window
    if steps < 1:
        raise ValueError('sequences of %d frames hold no window of %d and a frame to spare' % (T, window))
    starts = [(i, s) for i in range(n) for s in range(steps)]
    states, apps = [], []
    for at in range(0, len(starts), chunk):
        part = starts[at:at + chunk]
        x = torch.stack([X[i, s:s + window] for i, s in part]).to(device).contiguous()
        a = torch.stack([actions[i, s:s + window] for i, s in part]).to(device)
        _, prop, _ = state_model(x, 0, actions=a, pretrain=False)
        if prop.get('obj_appearances') is None:
            raise ValueError('load_and_encode orders the objects by their appearance: the model needs debug_core_appearance or '
                             'debug_match_appearance')
        z, app = red_first(prop['z'][:, -1].float(), prop['obj_appearances'][:, -1].float())
        states.append(z)
        apps.append(app)
    return torch.cat(states).contiguous(), torch.cat(apps).contiguous()
