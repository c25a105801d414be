"""Record what the control kernels compute, bit for bit, as the fixture of tests/test_gpu_control_bits.py: the reward head's forward
(reward_head_fwd_k), one planning expansion (plan_prep_k, plan_finish_k<16|32|64>) and the imagined PPO collection
(ppo_collect_model_k, ppo_collect_model_one_k, ppo_collect_model_cl_k<16|64>) -- the kernels that run the reward head's forward, its
table staging, the one-hot embedding and the policy step between two imagined steps, on shared code or on their own text of it.

Run on the GPU with the build whose results are to be the yardstick (the parent of a change that must not move a bit):

    python tools/make_control_bits_goldens.py [out.npz]        # default: tests/golden/g29_control_bits.npz

The fixture was recorded on commit e382c2c ("PPO on cl = 16 and 64 models: imagined collection in one launch"), before the
reward head's layout and dots, the argument block and the action embedding moved into shared headers, and is not recorded again for
that change.

Only public ops.* calls: ops.reward_head, ops.plan_expand(want_rewards=True), ops.ppo_collect_model.  One thing reaches below that
surface: ops.reward_head returns the reward alone, so the saved H0, Q, A1, A2 are read from its autograd node (saved_tensors[3], cut as
stove_reward_head_saved_floats lays the buffer out: H0 | Q | A1 | A2).  A change to how ops._RewardHeadFn saves that buffer has to be
followed in run_reward_head(); the digests of the four arrays themselves do not depend on how they are packed.  Models, policies and tables are the seeded builders of tests/ppo_model_cases.py, tests/ppo_model_cl_cases.py and
tests/plan_cl_cases.py; the states are drawn on the CPU here.  Per case the fixture holds the small inputs themselves, the SHA-256 of
every weight tensor (`<case>/w/...`) and the SHA-256 of every output (`<case>/out/...`): equal digests are equal bits, shape and
dtype.  Every case is run twice and must repeat itself bit for bit before it is recorded.
"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tests', 'golden')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'g29_control_bits.npz')
DEV = 'cuda:0'
WIDTHS = (16, 32, 64)
ITEMS = 5                                # reward head: more than one block's four waves
M, A, L, D, LEN_S, CAP = 2, 9, 2, 2, (1, 2), 10
B, S = 3, 3
# policy head width and depth per object count: one object (a kernel of its own at cl = 32), a wave per row, half-wave rows, and the
# widest policy, whose image is not staged
POLICY = {1: (32, False), 3: (64, False), 5: (64, True), 6: (128, True)}
COLLECT_KEYS = ('z_pred', 'pred', 'obs', 'actions', 'rewards', 'values', 'logp', 'next_value', 'returns', 'status')


def reward_head_cases():
    return [1, 3]


def plan_cases():
    """(cl, N, a bad leaf index in tree 1)"""
    return [(cl, n, False) for cl in WIDTHS for n in ((1, 3, 6) if cl == 32 else (1, 3))] + [(cl, 3, True) for cl in WIDTHS]


def collect_cases():
    """(cl, N, elu, trajectory 1 starts from a NaN state)"""
    out = []
    for cl in WIDTHS:
        out += [(cl, n, False, False) for n in ((1, 3, 5, 6) if cl == 32 else (1, 3, 6))]
        out += [(cl, 3, True, False), (cl, 3, False, True)]
    return out


def plan_key(cl, n, bad):
    return 'plan_cl%d_n%d%s' % (cl, n, '_bad' if bad else '')


def collect_key(cl, n, elu, nan):
    return 'collect_cl%d_n%d%s%s' % (cl, n, '_elu' if elu else '', '_nan' if nan else '')


def digest(t):
    """SHA-256 of a tensor's bytes (shape and dtype included) as 32 uint8"""
    a = np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t)
    h = hashlib.sha256(('%s%s' % (a.dtype, a.shape)).encode())
    h.update(a.tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


def model(cl, n, elu):
    """the seeded model of the shared cases: no appearance at one object, three floats otherwise"""
    app = 0 if n == 1 else 3
    if cl == 32:
        import ppo_model_cases as C
        return C.model(n, app, 'leaky_relu' if elu else 'relu'), app
    import ppo_model_cl_cases as C
    return C.model(cl, n, app, elu), app


def weights(st):
    """emb_w, emb_b, gnn image, reward-head block on the device"""
    import ppo_model_cases as C
    return C.weights(st)


def _weight_digests(names, tensors):
    return {'w/' + k: digest(t) for k, t in zip(names, tensors)}


# ------------------------------------------------------------------------------------------------ the reward head
def reward_head_inputs(n):
    g = np.random.default_rng(2900 + n)
    return {'pred': (1.5 * g.standard_normal((ITEMS, n, 32))).astype(np.float32)}


def run_reward_head(inp):
    """-> (outputs: reward and the saved H0, Q, A1, A2; weight digests)"""
    from stove_amd import ops
    st, _ = model(32, 3, False)
    h0, h1 = st.dyn.reward_head0, st.dyn.reward_head1
    params = [p.detach() for p in (h0[0].weight, h0[0].bias, h0[2].weight, h0[2].bias, h1[0].weight, h1[0].bias, h1[2].weight, h1[2].bias,
                                   h1[4].weight, h1[4].bias)]
    pred = torch.from_numpy(inp['pred']).to(DEV).requires_grad_()
    items, n = pred.shape[:2]
    r = ops.reward_head(pred, params)
    saved = r.grad_fn.next_functions[0][0].saved_tensors[3]          # H0 | Q | A1 | A2 (and one float of slack)
    torch.cuda.synchronize()
    cuts = np.cumsum([0, items * n * 32, items * 32, items * 16, items * 8])
    out = {'reward': r.detach().cpu()}
    out.update({k: saved[cuts[i]:cuts[i + 1]].cpu() for i, k in enumerate(('H0', 'Q', 'A1', 'A2'))})
    return out, {'w/rh': digest(torch.cat([p.float().reshape(-1) for p in params]))}


# ------------------------------------------------------------------------------------------------ one planning expansion
def plan_inputs(cl, n, bad):
    import plan_cl_cases as PC
    app_dim = 0 if n == 1 else 3
    g = torch.Generator().manual_seed(29000 + 100 * cl + n)
    z, app = PC.draw_states(g, M, n, cl, app_dim, 0.9)
    acts = torch.randint(0, A, (M * A, L), generator=g)
    inp = {'z': z.float().numpy(), 'acts': acts.numpy().astype(np.int32), 'leaf': np.array([0, CAP if bad else 0], dtype=np.int32)}
    if app is not None:
        inp['app'] = app.float().numpy()
    return inp


def run_plan(cl, n, inp):
    from stove_amd import ops
    st, _ = model(cl, n, False)
    w = weights(st)
    pool = torch.full((M, CAP, n, cl // 2 + 2), float('nan'))
    pool[:, 0] = torch.from_numpy(inp['z'])
    pool = pool.to(DEV)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)                     # noqa: E731
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)                        # noqa: E731
    q, rf, rr = ops.plan_expand(pool, dev(inp['leaf']), i32([1] * M), i32(LEN_S), dev(inp['app']) if 'app' in inp else None, dev(inp['acts']),
                                *w, D, 2, st.dyn.use_elu, st.dyn.loop_consts(), 0.95, want_rewards=True)
    torch.cuda.synchronize()
    return {'q': q.cpu(), 'r_first': rf.cpu(), 'r_roll': rr.cpu(), 'pool': pool.cpu()}, _weight_digests(('emb_w', 'emb_b', 'gnn', 'rh'), w)


# ------------------------------------------------------------------------------------------------ the imagined collection
def collect_inputs(cl, n, nan):
    from stove_amd.rl.collect import uniforms
    app_dim = 0 if n == 1 else 3
    rs = np.random.RandomState(29500 + 10 * n + cl)
    z0 = np.concatenate([np.full((B, n, 2), 0.1), rs.uniform(-0.7, 0.7, (B, n, 2)), rs.uniform(-0.1, 0.1, (B, n, 2)),
                         rs.uniform(-0.5, 0.5, (B, n, cl // 2 - 4))], axis=2).astype(np.float32)
    inp = {'u': np.array(uniforms(B, S, 2900 + n))}
    if app_dim:
        inp['app'] = rs.uniform(0, 1, (B, n, app_dim)).astype(np.float32)
    if nan:
        z0[1] = np.nan
    inp['z0'] = z0
    return inp


def run_collect(cl, n, elu, inp, want_pred):
    import ppo_cases as P
    from stove_amd import ops
    st, _ = model(cl, n, elu)
    w = weights(st)
    H, deep = POLICY[n]
    params = P.policy(n, H, deep).flat_params().to(DEV)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)                     # noqa: E731
    out = ops.ppo_collect_model(dev(inp['z0']), dev(inp['app']) if 'app' in inp else None, params, *w, dev(inp['u']), H, deep, 2, st.dyn.use_elu,
                                st.dyn.loop_consts(), 10.0, 0.95, want_pred=want_pred)
    torch.cuda.synchronize()
    res = {k: out[k].cpu() for k in COLLECT_KEYS if k != 'pred' or want_pred}
    return res, _weight_digests(('emb_w', 'emb_b', 'gnn', 'rh', 'policy'), w + (params,))


def run_collect_both(cl, n, elu, inp):
    """without and with `pred`: the second run's outputs under 'p/...'"""
    a, wd = run_collect(cl, n, elu, inp, False)
    b, _ = run_collect(cl, n, elu, inp, True)
    a.update({'p/' + k: v for k, v in b.items()})
    return a, wd


def _same(a, b):
    """bitwise (NaN included)"""
    return a.dtype == b.dtype and a.shape == b.shape and a.numpy().tobytes() == b.numpy().tobytes()


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    fix = {}

    def record(key, inp, fn):
        (a, wd), (b, _) = fn(), fn()
        for k in a:
            assert _same(a[k], b[k]), ('not repeatable', key, k)
        for k, v in inp.items():
            fix[key + '/in/' + k] = v
        for k, v in wd.items():
            fix[key + '/' + k] = v
        for k, v in a.items():
            fix[key + '/out/' + k] = digest(v)
        return a
    for n in reward_head_cases():
        inp = reward_head_inputs(n)
        res = record('rh_n%d' % n, inp, lambda: run_reward_head(inp))
        assert all(bool(torch.isfinite(v).all()) for v in res.values())
    for cl, n, bad in plan_cases():
        inp = plan_inputs(cl, n, bad)
        res = record(plan_key(cl, n, bad), inp, lambda: run_plan(cl, n, inp))
        assert bool(torch.isfinite(res['q'][0]).all()) and bool(torch.isnan(res['q'][1]).all()) == bad
    for cl, n, elu, nan in collect_cases():
        inp = collect_inputs(cl, n, nan)
        res = record(collect_key(cl, n, elu, nan), inp, lambda: run_collect_both(cl, n, elu, inp))
        assert res['status'].tolist() == ([0, 3, 0] if nan else [0, 0, 0]), (cl, n, elu, nan, res['status'])
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez_compressed(out_path, **fix)
    print('%s: %d arrays, %d bytes' % (out_path, len(fix), os.path.getsize(out_path)))


if __name__ == '__main__':
    main()
