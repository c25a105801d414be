"""The training step at the shapes that are trained and benchmarked -- BASELINE's (256 sequences x 100 frames) and the reference's
default training shape (256 clips x 8 frames) -- against the float64 oracle, row by row and gradient by gradient.

The paths these shapes take are picked by batch size: two encoder row chunks (the second on a side stream), the held-back object-SPN
table gradients (objspn_tablegrad_under_k: N <= 4 and >= 16 384 glimpses with the parameter stream), the small-tile recurrent products
and the split-K dh of the default shape, the multi-pass frame loop of the background SPN's backward.  A batch of K = 32 distinct
sequences, each on B / K rows scattered by a fixed permutation (helpers.replica_index), has the ELBO and the parameter gradients of
the 32-sequence batch (tests/test_batch_replication_cpu.py pins that on the oracle), so the oracle runs on 32 sequences only."""
import numpy as np
import pytest
import torch

import stove_oracle as O
from gpu_helpers import check, check_grad, err, fill_analytic
from helpers import oracle_stove, replica_index
from test_gpu_dynamics import CASES, DEV, make_cfg

pytestmark = pytest.mark.gpu

PRESET = {'n3': 'billiards', 'grav3': 'gravity', 'n6': 'multibilliards', 'ac3': 'avoidance'}
K = 32
ROLL = 92
_ORACLE = {}


def _oracle(name, T, regime):
    """(x, eps, actions, oracle step, oracle rollout) of the K distinct sequences, once per (workload, length, weight regime)"""
    key = (name, T, regime)
    if key not in _ORACLE:
        from stove_amd.envs import envs
        N = CASES[name]['num_obj']
        data = envs.synth_sequences(PRESET[name], K, T, seed0=700 + T)
        x = torch.from_numpy(data['X']).float()
        act = torch.from_numpy(data['action']).float() if 'action' in data else None
        eps = O.draw_eps(K, N, T, generator=torch.Generator().manual_seed(17 + T), dtype=torch.float64)
        ref = oracle_stove(CASES[name], x.double(), eps, act.double() if act is not None else None, regime)
        roll = None
        if T == 100:
            info = ref['info']
            with torch.no_grad():
                app = info['obj_appearances'][:, -1] if act is not None else None
                roll, _ = O.rollout(ref['c'], ref['params'], info['z'][:, -1], ROLL, act[:, :5].double() if act is not None else None, app)
        _ORACLE[key] = (x, eps, act, ref, roll)
    return _ORACLE[key]


def _same_bits_per_copy(t, src):
    """every row holds exactly the bits of the first row of its sequence"""
    first = np.zeros(K, dtype=np.int64)
    for b in range(len(src) - 1, -1, -1):
        first[src[b]] = b
    return torch.equal(t, t[torch.as_tensor(first[src], device=t.device)])


# The reference's own float32 run against its float64 run on the 'init' regime at 256 x 100 (this test's batch, oracle in float32 at
# all 256 rows against float64 at the 32 distinct sequences): with the reference's initial weights the objects of a frame are nearly
# alike, and at three objects float32 rounding alone moves z by 6e-3 of its largest entry -- the kernels land on the same values
# (6.3e-3); at six objects the gap stays below the 'analytic' bars.  The 'init' bars are 3x these gaps where they exceed the
# 'analytic' ones.
INIT_FP32_GAP = {
    'n3': dict(elbo_rel=1.42e-6, z=6.35e-3, z_dyn=1.66e-3, z_sup=1.17e-2, grad=2.64e-3, grad_l2=2.24e-3, grad_small=4.58e-2),
    'n6': dict(elbo_rel=5.9e-8, z=3.3e-7, z_dyn=5.5e-7, z_sup=2.7e-6, grad=3.3e-5, grad_l2=2.2e-5, grad_small=1.1e-3),
}


def _bar(name, regime, key, bar):
    return max(bar, 3.0 * INIT_FP32_GAP[name][key]) if regime == 'init' else bar


CASES_LB = ([(name, B, T, 'analytic') for name in CASES for B, T in ((256, 100), (256, 8))]
            + [(name, 256, 100, 'init') for name in ('n3', 'n6')])


@pytest.mark.parametrize('overlap', [True, False], ids=['overlap', 'one_stream'])
@pytest.mark.parametrize('name,B,T,regime', CASES_LB, ids=['%s-%dx%d-%s' % c for c in CASES_LB])
def test_training_step_at_full_size_against_the_oracle(name, B, T, regime, overlap):
    """ELBO, z / z_dyn / z_sup of all B rows, rewards, the 92-step rollout and every parameter gradient of the production model
    (fused kernels, flat parameter arena) against the oracle on the K distinct sequences; copies of a sequence bit for bit equal."""
    from stove_amd import settings
    from stove_amd.arena import ParamArena
    from stove_amd.video_prediction.stove import Stove
    x, eps, act, ref, roll = _oracle(name, T, regime)
    src = replica_index(B, K, seed=B * T)
    idx = torch.as_tensor(src)
    st = fill_analytic(Stove(make_cfg(fused_dynamics=True, fused_state=True, fused_elbo=True, **CASES[name])), '', regime).to(DEV)
    ar = ParamArena(st)
    assert ar.has_spn and ar.has_gnn
    table = {'latent': eps['latent'][..., 0][idx].float().to(DEV), 'std': eps['std'][..., 0][idx].float().to(DEV),
             'steps': torch.stack(eps['steps'], 1)[idx].float().to(DEV)}
    st.noise_fn = lambda kind, shape: table[kind].reshape(shape)
    actions = act[idx].to(DEV) if act is not None else None
    prev = settings.set_overlap(overlap)
    try:
        elbo, prop, rewards = st(x[idx].to(DEV), 0, actions)
        loss = -elbo
        if actions is not None:
            loss = loss + 3.0 * (rewards ** 2).mean()
        loss.backward()
        torch.cuda.synchronize()
        zp = None
        if roll is not None:
            with torch.no_grad():
                zp, _ = st.rollout(prop['z'][:, -1], num=ROLL, actions=actions[:, :5] if actions is not None else None,
                                   appearance=prop['obj_appearances'][:, -1] if actions is not None else None)
            torch.cuda.synchronize()
    finally:
        settings.set_overlap(prev)
    tag = 'fullbatch.T%d' % T + ('' if regime == 'analytic' else '.%s.%s' % (regime, name))
    info = ref['info']
    check(tag + '.elbo_rel', abs(float(elbo) - float(ref['elbo'])) / abs(float(ref['elbo'])), _bar(name, regime, 'elbo_rel', 1.5e-6))
    outs = {k: prop[k] for k in ('z', 'z_dyn', 'z_sup')}
    for k in outs:
        assert prop[k].shape[0] == B
        check(tag + '.' + k, err(prop[k], info[k][idx]), _bar(name, regime, k, 8e-6 if k == 'z_sup' else 3e-6))
    if actions is not None:
        check(tag + '.rewards', err(rewards, ref['rewards'][idx]), 1e-6)
        outs['rewards'] = rewards
    if zp is not None:
        check(tag + '.rollout_z', err(zp, roll[idx]), 3e-6)
        outs['rollout_z'] = zp
    for k, t in outs.items():                          # copies of one sequence: the same bits, wherever they sit in the batch
        assert _same_bits_per_copy(t.detach(), src), k
    n = 0
    for k, p in st.named_parameters():
        g_ref = ref['grads'].get(k)
        if g_ref is None:
            continue
        assert p.grad is not None, k
        check_grad(tag + '.grad', p.grad, g_ref, _bar(name, regime, 'grad', 3e-4), _bar(name, regime, 'grad_l2', 3.5e-4),
                   _bar(name, regime, 'grad_small', 4e-3))
        n += 1
    assert n == len(ref['grads']) and n > 100
