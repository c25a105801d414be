"""Record what the object SPN's table-gradient kernels (csrc/spn_obj.hip: objspn_tablegrad_under_k, objspn_tablegrad_k) compute, bit
for bit, as the fixture of tests/test_gpu_tablegrad_bits.py.

Run on the GPU with the build whose results are to be the yardstick (the parent of a change that must not move a bit; another build
is selected with STOVE_LIB, as tools/ab_lib.sh does):

    python tools/make_tablegrad_bits_goldens.py [out.npz]        # default: tests/golden/g30_tablegrad_bits.npz

Per case the call is the scene likelihood's training pair: stove_scene_fwd_from (the object SPN forward + backward at unit upstream
gradient, which leaves the scratch the table gradients are formed from) and stove_scene_bwd_overlap with a parameter stream distinct
from the main one (ops.scene_likelihood with a sink, overlap on) -- for at most four objects and at least 16 384 glimpses the held-back
objspn_tablegrad_under_k, otherwise the wide objspn_tablegrad_k.  The inputs are large (16 384 frames are 64 MB), so the fixture
holds their SEEDS: frames in [0, 1], valid z and a non-constant dll from torch's CPU generator, tables from the analytic fill.  Of
the results it holds the SHA-256 of the bytes (digest()): the three object-table gradients, and dz and the two background-table
gradients as a check that nothing else moved.  Every case is run twice and must repeat itself bit for bit before it is recorded.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tests', 'golden')):
    if p not in sys.path:
        sys.path.insert(0, p)

FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'g30_tablegrad_bits.npz')
OUTPUTS = ('g_obj_coef', 'g_obj_wsum', 'g_obj_wroot', 'dz', 'g_bg_coef', 'g_bg_wroot')
CHUNKS = 40                              # chunk count of the under path (objspn_backward_params)
LATE = 16384                             # kLateTableGradGlimpses (csrc/capi.hip)
# (objects, frames): glimpses = objects x frames in batches of 64, batch b belongs to chunk b mod 40
UNDER_CASES = ((1, 16384),               # 256 batches: 16 chunks get 7 batches, 24 get 6
               (3, 5462),                # 257 batches, the last with 2 live samples
               (2, 8200),                # the last batch with 16 live samples
               (4, 4106),                # the last batch with 40 live samples
               (4, 4480))                # 280 batches: every chunk gets 7
WIDE_CASES = ((3, 43),                   # 3 batches: fewer than the wide kernel's chunk count
              (6, 11))                   # six objects, 2 batches


def cases():
    return list(UNDER_CASES + WIDE_CASES)


def key(n_obj, nf):
    return 'n%d_f%d' % (n_obj, nf)


def case_seed(n_obj, nf):
    return 7000 + 13 * n_obj + nf


def digest(t):
    """SHA-256 of a tensor's bytes (shape and dtype included) as 32 uint8"""
    import hashlib
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    h = hashlib.sha256(('%s%s' % (a.dtype, a.shape)).encode())
    h.update(a.tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


def make_inputs(n_obj, nf, seed):
    """CPU-seeded: frames (nf, 1024) in [0, 1], z (nf * n_obj, 4) = [sx, sy, x, y] inside the model's ranges, dll (nf,) in [0.5, 1.5)"""
    g = torch.Generator().manual_seed(int(seed))
    frames = torch.rand(nf, 1024, generator=g) ** 2
    z = torch.zeros(nf, n_obj, 4)
    z[..., 0] = 0.1 + 0.6 * torch.rand(nf, n_obj, generator=g)
    z[..., 1] = z[..., 0] * (0.75 + 0.5 * torch.rand(nf, n_obj, generator=g))
    z[..., 2:] = 1.9 * torch.rand(nf, n_obj, 2, generator=g) - 0.95
    dll = 0.5 + torch.rand(nf, generator=g)
    return frames, z.flatten(0, 1).contiguous(), dll


def make_supair(n_obj, device):
    """the scene model with the analytic table fill (tests/golden/analytic_weights.py)"""
    from gpu_helpers import fill_analytic
    from stove_amd.video_prediction.config import StoveConfig
    from stove_amd.video_prediction.supair import Supair
    cfg = StoveConfig()
    cfg.num_obj, cfg.width, cfg.height = n_obj, 32, 32
    cfg.device, cfg.dtype, cfg.random_seed = torch.device(device), torch.float32, 42
    cfg.action_conditioned, cfg.action_space = False, None
    if n_obj != 3:
        cfg.debug_match_objects = 'greedy'
    return fill_analytic(Supair(cfg), 'sup.').to(device)


def run_case(sup, n_obj, nf, seed, device):
    """-> {name: CPU tensor} of OUTPUTS; the table gradients come through the sink of the parameter-stream path"""
    from stove_amd import _lib, ops, settings
    lib = _lib.load()
    frames, z, dll = (t.to(device) for t in make_inputs(n_obj, nf, seed))
    obj_tabs = tuple(t.detach() for t in sup.obj_spn.tables())
    bg_tabs = tuple(t.detach() for t in sup.bg_spn.tables())
    dense = torch.empty(lib.stove_bg_dense_floats(), dtype=torch.float32, device=device)
    _lib.check(lib.stove_bg_dense(bg_tabs[2].data_ptr(), bg_tabs[0].data_ptr(), dense.data_ptr(), _lib.stream()), 'stove_bg_dense')
    got = []
    prev = settings.set_overlap(True)
    try:
        zz = z.clone().requires_grad_()
        ll, _ = ops.scene_likelihood(frames, zz, obj_tabs, (*bg_tabs, dense), n_obj, sup.c.overlap_beta,
                                     sink=lambda gr: got.extend(t.clone() for t in gr))
        (ll * dll).sum().backward()
        torch.cuda.synchronize()
    finally:
        settings.set_overlap(prev)
    assert len(got) == 5
    res = {'g_obj_coef': got[0], 'g_obj_wsum': got[1], 'g_obj_wroot': got[2], 'g_bg_coef': got[3], 'g_bg_wroot': got[4], 'dz': zz.grad}
    return {k: v.cpu() for k, v in res.items()}


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    dev = 'cuda:0'
    fix = {}
    sups = {}
    for n_obj, nf in cases():
        sup = sups.setdefault(n_obj, make_supair(n_obj, dev))
        seed = case_seed(n_obj, nf)
        a, b = run_case(sup, n_obj, nf, seed, dev), run_case(sup, n_obj, nf, seed, dev)
        for k in OUTPUTS:
            assert torch.equal(a[k], b[k]), ('not repeatable', key(n_obj, nf), k)
            assert bool(torch.isfinite(a[k]).all()), ('not finite', key(n_obj, nf), k)
            assert float(a[k].abs().max()) > 0, ('all zero', key(n_obj, nf), k)
            fix[key(n_obj, nf) + '/' + k] = digest(a[k])
        fix[key(n_obj, nf) + '/seed'] = np.array([seed], dtype=np.int64)
        print(key(n_obj, nf), ' '.join('%s=%s' % (k, bytes(fix[key(n_obj, nf) + '/' + k][:4]).hex()) for k in OUTPUTS), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez_compressed(out_path, **fix)
    print('%s: %d arrays, %d bytes' % (out_path, len(fix), os.path.getsize(out_path)))


if __name__ == '__main__':
    main()
