"""The premise of the full-size parity tests (tests/test_gpu_large_batch.py): a batch of K distinct sequences, each repeated R times at
rows scattered by helpers.replica_index, has the ELBO and the parameter gradients of the K-sequence batch (the ELBO is a mean over
the batch, oracle/stove_oracle.py stove_forward, and sequences are independent), and every copy's latents are its source row's.  If
the model ever gains a batch-coupled term, this fails first.  CPU only: the float64 oracle against itself."""
import numpy as np
import pytest
import torch

import stove_oracle as O
from helpers import oracle_stove, replica_counts, replica_index, replicate_eps
from test_gpu_dynamics import CASES

PRESET = {'n3': 'billiards', 'grav3': 'gravity', 'n6': 'multibilliards', 'ac3': 'avoidance'}


def test_replica_index_places_every_item_evenly_without_structure():
    for n, K in ((256, 32), (25600, 32), (5462, 331), (176000, 331), (263144, 997)):
        src = replica_index(n, K, seed=n)
        cnt = replica_counts(src, K)
        assert src.shape == (n,) and cnt.min() == n // K and cnt.max() == -(-n // K)
        assert np.array_equal(src, replica_index(n, K, seed=n))                  # fixed
        r = np.arange(n)
        # an indexing error that reads another row -- a shift (e.g. the second half of a row-chunked product reading the first), a
        # row modulo a block size, or a block of rows read in the wrong order -- lands on another item on nearly every row
        wrong = [(r + s) % n for s in (1, 2, 32, 64, 256, n // 2, n - 1)] + [r % m for m in (32, 64, 256)] + [np.where((r ^ m) < n, r ^ m, r) for m in (1, 63)]
        for rr in wrong:
            moved = rr != r                                     # (rows the error leaves in place read the right item anyway)
            if not moved.any():
                continue
            same = float((src[rr] == src)[moved].mean())
            assert same < 0.1 + 1.5 / K, same
        # no block structure: neighbouring rows do not share an item more often than chance
        assert float((src[1:] == src[:-1]).mean()) < 3.0 / K


@pytest.mark.parametrize('name', ['n3', 'ac3'])
def test_replicated_batch_has_the_gradients_of_its_distinct_sequences(name):
    from stove_amd.envs import envs
    K, R, T = 3, 2, 6
    N = CASES[name]['num_obj']
    data = envs.synth_sequences(PRESET[name], K, T, seed0=41)
    x = torch.from_numpy(data['X']).double()
    act = torch.from_numpy(data['action']).double() if 'action' in data else None
    eps = O.draw_eps(K, N, T, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    src = replica_index(K * R, K, seed=1)
    assert sorted(np.bincount(src)) == [R] * K and not np.array_equal(src, np.arange(K * R) % K)
    idx = torch.as_tensor(src)
    small = oracle_stove(CASES[name], x, eps, act)
    big = oracle_stove(CASES[name], x[idx], replicate_eps(eps, src), act[idx] if act is not None else None)
    assert abs(float(big['elbo']) - float(small['elbo'])) <= 1e-12 * abs(float(small['elbo']))
    assert set(big['grads']) == set(small['grads']) and len(small['grads']) > 100
    if act is not None:
        assert any('reward' in k for k in small['grads'])                       # the reward head is in the loss
        assert torch.equal(big['rewards'], small['rewards'][idx])
    for k, gs in small['grads'].items():
        d = float((big['grads'][k] - gs).abs().max())
        assert d <= 1e-12 * (float(gs.abs().max()) + 1e-300), (k, d)
    for k in ('z', 'z_dyn', 'z_sup'):
        # (to 1e-12, not bit for bit: the host BLAS blocks a product of 12 rows otherwise than one of 6)
        ref = small['info'][k][idx]
        assert float((big['info'][k] - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), k
