"""Operators past every size threshold and grid cap of their launchers, against the float64 oracle: the scene likelihood one frame
below and at the held-back table-gradient threshold (kLateTableGradGlimpses, csrc/capi.hip) and past the tile kernels' and the
object SPN's grid caps, the object-SPN operator past its 4 096-workgroup cap, and the recognition network at the default training
shape (small tile, split-K dh), in two row chunks and unchunked past the LSTM cell kernels' grid cap.

K distinct frames / glimpses / rows fill the n rows of the batch, each on about n / K rows placed by a fixed permutation
(helpers.replica_index): outputs are compared row by row to their item's, the batch-summed parameter gradients to the oracle's
gradient of the same loss with item k weighted by the number of rows that hold it."""
import pytest
import torch

import stove_oracle as O
from gpu_helpers import check, check_grad, err
from helpers import replica_counts, replica_index
from test_gpu_spn import FWD_TOL, GRAD_TOL, _oracle_spn, _spn_pair, _supair_pair

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _first_rows(src, K):
    import numpy as np
    first = np.zeros(K, dtype=np.int64)
    for b in range(len(src) - 1, -1, -1):
        first[src[b]] = b
    return torch.as_tensor(first[src], device=DEV)


def _scene_case(n_obj, nf, tile_modes, key):
    from stove_amd import _lib, ops, settings
    K = 331
    extra = {'debug_match_objects': 'greedy'} if n_obj != 3 else {}
    c, structs, params, sup = _supair_pair(n_obj, **extra)
    g = torch.Generator().manual_seed(1000 + n_obj)
    x64 = torch.rand(K, 1, 1, 32, 32, generator=g, dtype=torch.float64) ** 2
    z64 = torch.zeros(K, n_obj, 4, dtype=torch.float64)
    z64[..., 0] = 0.1 + 0.6 * torch.rand(K, n_obj, generator=g, dtype=torch.float64)
    z64[..., 1] = z64[..., 0] * (0.75 + 0.5 * torch.rand(K, n_obj, generator=g, dtype=torch.float64))
    z64[..., 2:] = 1.9 * torch.rand(K, n_obj, 2, generator=g, dtype=torch.float64) - 0.95
    w64 = torch.linspace(0.5, 1.5, K, dtype=torch.float64)
    src = replica_index(nf, K, seed=nf * n_obj)
    cnt = torch.as_tensor(replica_counts(src, K), dtype=torch.float64)
    idx = torch.as_tensor(src)
    z_o = z64.flatten(0, 1).clone().requires_grad_()
    ll_o = O.scene_likelihood(c, params, structs, x64, z_o)
    (ll_o * w64 * cnt).sum().backward()
    dz_o = z_o.grad.view(K, n_obj, 4) / cnt.view(K, 1, 1)
    frames = x64.view(K, 1024)[idx].float().to(DEV)
    z = z64[idx].float().reshape(-1, 4).to(DEV)
    w = w64[idx].float().to(DEV)
    lib = _lib.load()
    prev = settings.set_overlap(True)
    try:
        for mode in tile_modes:
            if mode is not None:
                lib.stove_set_tile_lds(mode)
            for stream in ('one_stream', 'param_stream'):
                sup.zero_grad()
                obj_tabs, bg_tabs = sup.obj_spn.tables(), sup.bg_spn.tables()
                zz = z.clone().requires_grad_()
                if stream == 'one_stream':       # stove_scene_bwd: the immediate objspn_tablegrad_k, gradients through autograd
                    ll, _ = ops.scene_likelihood(frames, zz, obj_tabs, bg_tabs, n_obj, c.overlap_beta)
                    (ll * w).sum().backward()
                else:                            # stove_scene_bwd_overlap: parameter stream + sink (held back for N <= 4, >= 16 384 glimpses)
                    dense = torch.empty(lib.stove_bg_dense_floats(), dtype=torch.float32, device=DEV)
                    _lib.check(lib.stove_bg_dense(bg_tabs[2].data_ptr(), bg_tabs[0].data_ptr(), dense.data_ptr(), _lib.stream()), 'stove_bg_dense')
                    got = []
                    ll, _ = ops.scene_likelihood(frames, zz, tuple(t.detach() for t in obj_tabs), (*(t.detach() for t in bg_tabs), dense),
                                                 n_obj, c.overlap_beta, sink=lambda gr: got.extend(t.clone() for t in gr))
                    (ll * w).sum().backward()
                    torch.cuda.synchronize()
                    assert len(got) == 5
                    leaves = (*obj_tabs[:3], *bg_tabs[:2])
                    torch.autograd.backward(list(leaves), [gt.view_as(t) for gt, t in zip(got, leaves)])
                torch.cuda.synchronize()
                check(key + '.ll', err(ll, ll_o.detach()[idx]), FWD_TOL)
                dz = zz.grad.view(nf, n_obj, 4)
                check(key + '.dz', err(dz, dz_o[idx]), GRAD_TOL)
                # (copies of a frame are NOT held to the same bits here: the fused scene likelihood of one frame differs in the last
                # bits with the frame's row -- found by this test; every row is held to the oracle instead)
                n = 0
                for name, p in sup.named_parameters():
                    if 'encoder' in name:
                        continue
                    ref = params['sup.' + name].grad
                    if name.endswith('output_vector.params'):
                        check(key + '.grad_root', err(p.grad, ref), GRAD_TOL)      # (softmax root: entries cancel, max-norm only)
                    else:
                        check_grad(key + '.grad_param', p.grad, ref, GRAD_TOL, 2.5e-4, 5e-3)
                    n += 1
                assert n > 60
    finally:
        lib.stove_set_tile_lds(1)
        settings.set_overlap(prev)


# (glimpses = frames x objects: 16 383 / 16 384, one frame below and at kLateTableGradGlimpses; four objects: scene_bwd_tail<6>)
@pytest.mark.parametrize('n_obj,nf', [(1, 16383), (1, 16384), (3, 5461), (3, 5462), (4, 4095), (4, 4096)])
def test_scene_likelihood_at_the_held_back_table_gradient_threshold(n_obj, nf):
    _scene_case(n_obj, nf, (None,), 'largeop.scene_late')


def test_scene_likelihood_past_the_grid_caps():
    """176 000 frames x 3 objects = 528 000 glimpses: past the object SPN kernels' 4 096 x 64 and the tile kernels' 8 192 x 64 glimpse
    caps (second grid-stride passes), with either tile kernel (lane per glimpse / lane per pixel)"""
    assert 176000 * 3 > 8192 * 64 > 4096 * 64
    _scene_case(3, 176000, (0, 2), 'largeop.scene_caps')


def test_object_spn_operator_past_its_grid_cap():
    """RatSpn.forward (ops.objspn_apply) on 4 096 x 64 + 1 000 glimpses: forward and every gradient past the 4 096-workgroup cap"""
    c, structs, params, spn = _spn_pair('obj')
    K, n = 997, 4096 * 64 + 1000
    g = torch.Generator().manual_seed(4)
    x64 = torch.rand(K, 100, generator=g, dtype=torch.float64)
    m64 = torch.rand(K, 100, generator=g, dtype=torch.float64) * 1.4 - 0.2
    m64[0] = 0.0
    w64 = torch.linspace(0.5, 1.5, K, dtype=torch.float64)
    src = replica_index(n, K, seed=n)
    cnt = torch.as_tensor(replica_counts(src, K), dtype=torch.float64)
    idx = torch.as_tensor(src)
    x_o, m_o = x64.clone().requires_grad_(), m64.clone().requires_grad_()
    out_o = _oracle_spn('obj', c, structs, params, x_o, m_o)
    (out_o[:, 0] * w64 * cnt).sum().backward()
    x_d = x64[idx].float().to(DEV).requires_grad_()
    m_d = m64[idx].float().to(DEV).requires_grad_()
    out_d = spn(x_d, m_d)
    assert out_d.shape == (n, 1)
    (out_d[:, 0] * w64[idx].float().to(DEV)).sum().backward()
    torch.cuda.synchronize()
    check('largeop.objspn.fwd', err(out_d, out_o.detach()[idx]), FWD_TOL)
    check('largeop.objspn.grad_x', err(x_d.grad, (x_o.grad / cnt.view(K, 1))[idx]), GRAD_TOL)
    check('largeop.objspn.grad_m', err(m_d.grad, (m_o.grad / cnt.view(K, 1))[idx]), GRAD_TOL)
    first = _first_rows(src, K)
    assert torch.equal(out_d, out_d[first]) and torch.equal(x_d.grad, x_d.grad[first]) and torch.equal(m_d.grad, m_d.grad[first])
    for name, p in spn.named_parameters():
        if name.startswith('output_vector'):
            continue
        check_grad('largeop.objspn.grad_param', p.grad, params['sup.obj_spn.' + name].grad, GRAD_TOL, 2.5e-4, 5e-3)


# 2 048 rows: the default training shape's 256 x 8 frames (small-M tile, split-K dh with the dense term riding the slice sum);
# 40 960: two row chunks, the second on the side stream, and a second pass of the LSTM cell kernels' grid in the backward;
# 33 004: unchunked (not a multiple of 256), past the cell kernels' 8 192 x 256-item cap at H = 256
@pytest.mark.parametrize('n', [2048, 40960, 33004])
def test_recognition_network_at_large_row_counts(n):
    from gpu_helpers import fill_analytic
    from helpers import oracle_setup
    from stove_amd import ops
    from stove_amd.arena import ParamArena
    from stove_amd.video_prediction.encoder import RnnStates
    from test_gpu_dynamics import make_cfg
    N, K = 3, 251
    assert (ops._enc_chunks(n, 1024, 256) is not None) == (n == 40960)
    c, structs, params = oracle_setup(torch.float64, num_obj=N)
    g = torch.Generator().manual_seed(n)
    x64 = (torch.rand(K, 1, 32, 32, generator=g, dtype=torch.float64) > 0.8).double() * torch.rand(K, 1, 32, 32, generator=g, dtype=torch.float64)
    w64 = torch.randn(K, N, 8, generator=g, dtype=torch.float64)
    src = replica_index(n, K, seed=n)
    cnt = torch.as_tensor(replica_counts(src, K), dtype=torch.float64)
    idx = torch.as_tensor(src)
    out_o = O.encoder_forward(c, params, x64)
    (out_o * w64 * cnt.view(K, 1, 1)).sum().backward()
    enc = fill_analytic(RnnStates(make_cfg(num_obj=N)), 'sup.encoder.').to(DEV)
    arena = ParamArena(enc)
    arena.zero()
    out = enc(x64[idx].float().to(DEV))
    (out * w64[idx].float().to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert out.shape == (n, N, 8)
    check('largeop.encoder.codes', err(out, out_o.detach()[idx]), 5e-6)
    assert torch.equal(out, out[_first_rows(src, K)])
    k = 0
    for name, p in enc.named_parameters():
        check_grad('largeop.encoder.grad', p.grad, params['sup.encoder.' + name].grad, 3e-4, 3.5e-4, 4e-3)
        k += 1
    assert k == 8
