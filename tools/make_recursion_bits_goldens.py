"""Record what the small-graph recursion kernels compute, bit for bit, as the fixture of tests/test_gpu_recursion_bits.py.

Run on the GPU with the build whose results are to be the yardstick (the parent of a change that must not move a bit):

    python tools/make_recursion_bits_goldens.py [out.npz]        # default: tests/golden/g28_recursion_bits.npz

The fixture holds, per case, the CPU-seeded inputs and the outputs of ops.dyn_loop (saving forward), of its backward (state
gradients and the weight gradients gnn_dw_small_k forms from the saved streams and the dY streams), of the mean rollout and of the
sampling rollout (draws given: states, scales, predictions and the draws' log-density).  The
outputs are recorded as the SHA-256 of their bytes (digest()): the weight gradients alone are 90 KB a case, 4 MB over the cases,
and equal digests are equal bits.  The weights are multiples of 2^-10 kept as int16 numerators; the cotangents of the backward are
a closed form (cotangent()), exact in any arithmetic.  Every case is run twice and must repeat itself bit for bit before it is
recorded.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'g28_recursion_bits.npz')
B = 3                                   # more than one workgroup
OBJECTS = (1, 2, 3, 4, 5, 6)
STEPS = (1, 2, 5)                       # a one-step loop, both parities, an odd count
AC_OBJECTS = (3, 6)                     # action-conditioned: 23 inputs per node, `pred` returned
ROLLOUT_STEPS = 3
PIECES = (0, 2, 5)                      # the five-step cases again as the pieces [0, 2) + [2, 5): run_loop_pieces, nothing recorded
CONSTS = (0.3, 0.04, 0.1)               # Dynamics.loop_consts() of the default configuration
OUTPUTS = ('z', 'zdyn', 'zdstd', 'mean', 'stdv', 'pred')
STATE_GRADS = ('dz1', 'dzsup', 'dzsstd', 'dextra')


def loop_cases():
    """(n_obj, steps, action-conditioned)"""
    return [(n, ts, 0) for n in OBJECTS for ts in STEPS] + [(n, ts, 1) for n in AC_OBJECTS for ts in STEPS]


def rollout_cases():
    return [(n, ac) for n in AC_OBJECTS for ac in (0, 1)]


def key(n, ts, ac, elu=None):
    return 'n%d_t%d_ac%d' % (n, ts, ac) + ('' if elu is None else ('_elu' if elu else '_relu'))


def make_weights(seed=2024):
    """int16 numerators (over 1024) of the W image and the vector image"""
    from stove_amd import ops
    g = np.random.default_rng(seed)
    return (g.integers(-128, 129, ops.GNN_W_FLOATS).astype(np.int16), g.integers(-128, 129, ops.GNN_V_FLOATS).astype(np.int16))


def image_from(w_num, v_num, device):
    """(w_img, v_img, wt_img) as ops.dyn_loop takes them, from the numerators; w_img and v_img are leaves that take gradients"""
    from stove_amd import ops
    w = torch.from_numpy(w_num.astype(np.float32) / 1024.0)
    wt = torch.empty_like(w)
    for off, out_f, k_f in ops._GNN_LAYERS:
        wt[off:off + out_f * k_f] = w[off:off + out_f * k_f].view(out_f, k_f).t().reshape(-1)
    v = torch.from_numpy(v_num.astype(np.float32) / 1024.0)
    return w.to(device).requires_grad_(), v.to(device).requires_grad_(), wt.to(device)


def make_inputs(n, ts, ac, seed):
    g = np.random.default_rng(seed)
    f = lambda a: a.astype(np.float32)                     # noqa: E731
    d = {'z1': f(g.random((B, n, 18)) - 0.5), 'zsup': f(g.random((B, ts, n, 6)) - 0.5),
         'zsstd': f(0.05 + 0.1 * g.random((B, ts, n, 6))), 'eps': f(g.standard_normal((B, ts, n, 18)))}
    if ac:
        d['extra'] = f(0.5 * g.standard_normal((B, ts, n, 7)))
    return d


def digest(t):
    """SHA-256 of a tensor's bytes (shape and dtype included) as 32 uint8"""
    import hashlib
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    h = hashlib.sha256(('%s%s' % (a.dtype, a.shape)).encode())
    h.update(a.tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


def cotangent(t, salt):
    """exact in float32: multiples of 1/64 in [-50/64, 50/64], another pattern per output"""
    i = torch.arange(t.numel(), dtype=torch.int64, device=t.device)
    return (((i * 37 + salt * 11) % 101 - 50).to(torch.float32) / 64.0).view(t.shape)


def run_loop(inp, image, elu, save=True):
    """-> dict of the outputs (and, saving, of every gradient) as CPU tensors"""
    from stove_amd import ops
    dev = image[0].device
    t = {k: torch.from_numpy(v).to(dev) for k, v in inp.items()}
    extra = t.get('extra')
    for p in image[:2]:
        p.grad = None
    if not save:
        with torch.no_grad():
            out = ops.dyn_loop(t['z1'], t['zsup'], t['zsstd'], t['eps'], extra, image, 2, elu, CONSTS, want_pred=extra is not None)
        return {k: o.cpu() for k, o in zip(OUTPUTS, out) if o.numel()}
    for k in ('z1', 'zsup', 'zsstd') + (('extra',) if extra is not None else ()):
        t[k].requires_grad_()
    out = ops.dyn_loop(t['z1'], t['zsup'], t['zsstd'], t['eps'], extra, image, 2, elu, CONSTS, want_pred=extra is not None)
    res = {k: o.detach().cpu() for k, o in zip(OUTPUTS, out) if o.numel()}
    loss = sum((o * cotangent(o, s)).sum() for s, (k, o) in enumerate(zip(OUTPUTS, out)) if o.numel() and k != 'zdstd')
    loss.backward()
    res.update(dz1=t['z1'].grad.cpu(), dzsup=t['zsup'].grad.cpu(), dzsstd=t['zsstd'].grad.cpu(), dW=image[0].grad.cpu(), dV=image[1].grad.cpu())
    if extra is not None:
        res['dextra'] = t['extra'].grad.cpu()
    return res


def run_loop_pieces(inp, image, elu, bounds=PIECES):
    """run_loop's saving call and its backward with the steps cut at `bounds`: the forward piece by piece into one set of outputs, the
    backward from the last piece to the first over the same streams, the state gradient handed on through the carry buffer
    (stove_debug_set_piece).  Small-graph kernels only, 2 .. 6 objects.  Same results as run_loop, names and all."""
    from stove_amd import _lib, ops
    from stove_amd._lib import check, ptr, stream
    lib = _lib.load()
    dev = image[0].device
    t = {k: torch.from_numpy(v).to(dev) for k, v in inp.items()}
    z1, zsup, zsstd, eps, extra = t['z1'], t['zsup'], t['zsstd'], t['eps'], t.get('extra')
    B, Ts, N = zsup.shape[:3]
    assert bounds[0] == 0 and 2 <= N <= 6          # (a last bound beyond Ts is the library's to refuse)
    pieces = list(zip(bounds[:-1], bounds[1:]))
    width = ops.gnn_width(32)
    params = width.image(image[0].detach(), image[1].detach(), image[2])
    sd = 16 + (extra.shape[-1] if extra is not None else 0)
    new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)                     # noqa: E731
    out = {k: new(B, Ts, N, d) for k, d in zip(OUTPUTS, (18, 16, 16, 18, 18, 32)) if k != 'pred' or extra is not None}
    act = new(lib.stove_dynloop_act_floats(B, Ts, N) + 1)
    carry = new(B, N, 18)
    dz1, dzsup, dzsstd = torch.empty_like(z1), torch.empty_like(zsup), torch.empty_like(zsstd)
    dextra = torch.empty_like(extra) if extra is not None else None
    g = new(lib.stove_gnn_grad_floats())
    ws = new(lib.stove_dynloop_bwd_ws_bytes_ts(B, Ts, N) // 4 + 1)
    tail = (B, Ts, N, sd, 2, int(elu)) + tuple(float(c) for c in CONSTS) + (stream(),)
    try:
        for a, b in pieces:
            lib.stove_debug_set_piece(a, b, ptr(carry))
            check(lib.stove_dynloop_fwd(ptr(z1), ptr(zsup), ptr(zsstd), ptr(eps), ptr(extra), ptr(params), ptr(out['z']), ptr(out['zdyn']),
                                        ptr(out['zdstd']), ptr(out['mean']), ptr(out['stdv']), ptr(out.get('pred')), ptr(act), *tail),
                  'stove_dynloop_fwd')
        cot = {k: cotangent(out[k], s) for s, k in enumerate(OUTPUTS) if k in out and k != 'zdstd'}
        for a, b in reversed(pieces):
            lib.stove_debug_set_piece(a, b, ptr(carry))
            check(lib.stove_dynloop_bwd(ptr(z1), ptr(zsup), ptr(zsstd), ptr(eps), ptr(extra), ptr(params), ptr(out['z']), ptr(act), ptr(cot['z']),
                                        ptr(cot['zdyn']), ptr(cot['mean']), ptr(cot['stdv']), ptr(cot.get('pred')), ptr(dz1), ptr(dzsup),
                                        ptr(dzsstd), ptr(dextra), ptr(g), ptr(ws), *tail), 'stove_dynloop_bwd')
    finally:
        lib.stove_debug_set_piece(0, 0, None)
    torch.cuda.synchronize(dev)
    dW, dV = width.split(g)
    res = {k: o.cpu() for k, o in out.items()}
    res.update(dz1=dz1.cpu(), dzsup=dzsup.cpu(), dzsstd=dzsstd.cpu(), dW=dW.cpu(), dV=dV.cpu())
    if dextra is not None:
        res['dextra'] = dextra.cpu()
    return res


def run_rollout(inp, image, elu, sample=False):
    """the mean rollout, or (sample) the sampling rollout on the draws inp['eps'] (B, steps, n, 16)"""
    from stove_amd import ops
    dev = image[0].device
    z_last = torch.from_numpy(inp['z1']).to(dev)
    extra = torch.from_numpy(inp['extra']).to(dev) if 'extra' in inp else None
    if sample:
        with torch.no_grad():
            z_pred, zstd, pred, log_q = ops.rollout(z_last, extra, image, ROLLOUT_STEPS, 2, elu, CONSTS, want_std=True, want_pred=extra is not None,
                                                    eps=torch.from_numpy(inp['eps']).to(dev), want_logq=True)
        res = {'z_pred': z_pred.cpu(), 'zstd': zstd.cpu(), 'log_q': log_q.cpu()}
        if extra is not None:
            res['pred'] = pred.cpu()
        return res
    with torch.no_grad():
        z_pred, zstd, pred = ops.rollout(z_last, extra, image, ROLLOUT_STEPS, 2, elu, CONSTS, want_std=True, want_pred=extra is not None)
    res = {'z_pred': z_pred.cpu(), 'zstd': zstd.cpu()}
    if pred is not None:
        res['pred'] = pred.cpu()
    return res


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    dev = torch.device('cuda:0')
    w_num, v_num = make_weights()
    image = image_from(w_num, v_num, dev)
    fix = {'w_num': w_num, 'v_num': v_num}
    seed = 100

    def twice(fn):
        a, b = fn(), fn()
        for k in a:
            assert torch.equal(a[k], b[k]), ('not repeatable', k)
            assert bool(torch.isfinite(a[k]).all()), ('not finite', k)
        return a
    for n, ts, ac in loop_cases():
        seed += 1
        inp = make_inputs(n, ts, ac, seed)
        for k, v in inp.items():
            fix[key(n, ts, ac) + '/' + k] = v
        for elu in (False, True):
            res = twice(lambda: run_loop(inp, image, elu))
            for k, v in res.items():
                fix[key(n, ts, ac, elu) + '/' + k] = digest(v)
    for n, ac in rollout_cases():
        seed += 1
        inp = make_inputs(n, ROLLOUT_STEPS, ac, seed)       # (extra: one action per step)
        for k in ('z1',) + (('extra',) if ac else ()):
            fix['roll_' + key(n, ROLLOUT_STEPS, ac) + '/' + k] = inp[k]
        for elu in (False, True):
            res = twice(lambda: run_rollout(inp, image, elu))
            for k, v in res.items():
                fix['roll_' + key(n, ROLLOUT_STEPS, ac, elu) + '/' + k] = digest(v)
    for n, ac in rollout_cases():                           # the sampling rollout: the draws are the loop's, state dims only
        seed += 1
        inp = make_inputs(n, ROLLOUT_STEPS, ac, seed)
        inp['eps'] = np.ascontiguousarray(inp['eps'][..., 2:])
        for k in ('z1', 'eps') + (('extra',) if ac else ()):
            fix['sroll_' + key(n, ROLLOUT_STEPS, ac) + '/' + k] = inp[k]
        for elu in (False, True):
            res = twice(lambda: run_rollout(inp, image, elu, sample=True))
            for k, v in res.items():
                fix['sroll_' + key(n, ROLLOUT_STEPS, ac, elu) + '/' + k] = digest(v)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez_compressed(out_path, **fix)
    print('%s: %d arrays, %d bytes' % (out_path, len(fix), os.path.getsize(out_path)))


if __name__ == '__main__':
    main()
