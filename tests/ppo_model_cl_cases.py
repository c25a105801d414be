"""Shared cases of the tests of the model-based PPO arm's collection on models of state-code length 16 and 64
(tests/test_ppo_model_cl_cpu.py, tests/test_gpu_ppo_model_cl.py), in the manner of tests/ppo_model_cases.py: the seeded shape cases,
their policies (ppo_cases.policy), a seeded untrained action-conditioned dynamics model per (cl, N, app_dim, activation) built on
plan_cl_cases.cl_cfg the way tests/test_gpu_plan_cl.py builds its models, start states that the model itself rolled out, and the
kernel's collection of each case (computed once per case, never modified)."""
import functools

import numpy as np
import torch

import plan_cl_cases as PC
import ppo_cases as P
from stove_amd.rl.collect import uniforms

DEV = 'cuda:0'
HW, DISCOUNT, MIN_MARGIN = 10.0, P.DISCOUNT, P.MIN_MARGIN
WIDTHS = PC.WIDTHS
FIRST_SEED = 4100
KEYS = ('z_pred', 'pred', 'obs', 'actions', 'rewards', 'values', 'logp', 'next_value', 'returns', 'status')
FLOATS = ('z_pred', 'pred', 'obs', 'rewards', 'values', 'logp', 'next_value', 'returns')


def _grid(cl):
    """(stem, B, S, N, H, deep, app_dim, elu) per width; debug_nonlinear 'leaky_relu' is the dynamics' ELU (Dynamics.use_elu)"""
    wide = PC.app_limit(cl)
    return (('b1_s1_n1_h32', 1, 1, 1, 32, False, 0, False),                    # no edges, no appearance, one step
            ('b3_s5_n3_h64', 3, 5, 3, 64, False, 3, False),                    # the workload's kind
            ('b3_s5_n3_h64_elu', 3, 5, 3, 64, False, 3, True),                 # the other activation of the dynamics
            ('b3_s5_n4_h40', 3, 5, 4, 40, False, 3, False),                    # H no multiple of 32
            ('b5_s6_n6_h128_deep', 5, 6, 6, 128, True, wide, False))           # most rows, widest policy (image not staged), sin_dim == cl


# name -> (cl, B, S, N, H, deep, app_dim, elu)
CASES = {'cl%d_%s' % (cl, row[0]): (cl,) + row[1:] for cl in WIDTHS for row in _grid(cl)}
# The seed of the u table, collect.uniforms(B, S, seed), per case: the first from FIRST_SEED on whose smallest decision margin in the host
# forest, on the kernel's own states, is >= MIN_MARGIN = 1e-9 (asserted by the GPU tests, no trajectory left out).  With float32
# uniforms a draw violates that with a chance of about 2e-8, so no seed had to be passed over: every case uses FIRST_SEED.
SEEDS = {name: FIRST_SEED for name in CASES}
PASSED_OVER = {}          # name -> the seeds below its own that missed the margin: none


def policy(name):
    cl, B, S, N, H, deep = CASES[name][:6]
    return P.policy(N, H, deep)


@functools.lru_cache(maxsize=None)
def model(cl, N, app_dim, elu):
    """an untrained, seeded action-conditioned dynamics model of state-code length cl on N objects, wrapped as planning's tests wrap
    theirs (Stove.rollout on the module); read only"""
    from test_gpu_dynamics import make_cfg
    from test_gpu_plan_counts import _Env
    from stove_amd.video_prediction.dynamics import Dynamics
    state = torch.get_rng_state()
    torch.manual_seed(cl)
    st = _Env(Dynamics(make_cfg(**PC.cl_cfg(cl, N, 9, app_dim, elu))).to(DEV))
    torch.set_rng_state(state)
    assert st.c.cl == cl and st.c.action_conditioned and st.dyn.use_elu == elu
    for p in st.parameters():
        p.requires_grad_(False)
    return st.eval()


def case_model(name):
    cl, B, S, N, H, deep, app_dim, elu = CASES[name]
    return model(cl, N, app_dim, elu)


def weights(st):
    """what stove_ppo_collect_model_cl reads of the model: embedding, GNN image, reward-head block (stove_plan_expand_cl's set)"""
    from stove_amd.mcts.mcts_stove import BatchedMCTSHandler
    with torch.no_grad():
        return BatchedMCTSHandler._fused_weights(st)


@functools.lru_cache(maxsize=None)
def start(name):
    """-> (z0 (B, N, cl/2 + 2), app (B, N, app_dim) or None) on the device: seeded states (scales 0.1, positions in +-0.7, velocities in
    +-0.1, latents in +-0.5) rolled two steps through the model under seeded actions, so that they lie where the model operates"""
    cl, B, S, N, H, deep, app_dim = CASES[name][:7]
    st = case_model(name)
    rs = np.random.RandomState(5200 + 10 * N + B + cl)
    z = np.concatenate([np.full((B, N, 2), 0.1), rs.uniform(-0.7, 0.7, (B, N, 2)), rs.uniform(-0.1, 0.1, (B, N, 2)),
                        rs.uniform(-0.5, 0.5, (B, N, cl // 2 - 4))], axis=2).astype(np.float32)
    app = torch.from_numpy(rs.uniform(0, 1, (B, N, app_dim)).astype(np.float32)).to(DEV) if app_dim else None
    acts = torch.nn.functional.one_hot(torch.from_numpy(rs.randint(0, 9, (B, 2))), 9).float().to(DEV)
    with torch.no_grad():
        z0 = st.rollout(torch.from_numpy(z).to(DEV), 2, actions=acts, appearance=app)[0][:, -1].contiguous()
    assert bool(torch.isfinite(z0).all()) and tuple(z0.shape) == (B, N, cl // 2 + 2)
    return z0, app


@functools.lru_cache(maxsize=None)
def table(name):
    """u (B, S) float32 in [0, 1); read only"""
    u = uniforms(CASES[name][1], CASES[name][2], SEEDS[name])
    u.setflags(write=False)
    return u


def shapes(name, B=None, S=None):
    cl, b, s, N = CASES[name][:4]
    B, S = (b if B is None else B), (s if S is None else S)
    return {'z_pred': (B, S, N, cl // 2 + 2), 'pred': (B, S, N, cl), 'obs': (B, S + 1, 4 * N), 'actions': (B, S), 'rewards': (B, S),
            'values': (B, S), 'logp': (B, S), 'next_value': (B,), 'returns': (B, S), 'status': (B,)}


def collect(name, z0=None, graph=False, B=None, S=None):
    """ops.ppo_collect_model on guarded device copies of the case's inputs (the first B trajectories and S steps of them, all by default);
    the outputs pre-filled with NaN / -77 -> (out dict of device tensors, every guarded buffer)"""
    from control_harness import guarded
    from stove_amd import ops
    cl, b, s, N, H, deep, app_dim = CASES[name][:7]
    B, S = (b if B is None else B), (s if S is None else S)
    st = case_model(name)
    z_start, app = start(name)
    buffers, out = {}, {}
    z0, buffers['z0'] = guarded((z_start if z0 is None else z0)[:B].cpu(), float('nan'))
    if app is not None:
        app, buffers['app'] = guarded(app[:B].cpu(), float('nan'))
    params, buffers['params'] = guarded(policy(name).flat_params(), float('nan'))
    u, buffers['u'] = guarded(torch.from_numpy(np.array(table(name)[:B, :S])), float('nan'))
    emb_w, emb_b, gnn, rh = weights(st)
    for k, shape in shapes(name, B, S).items():
        fill = torch.full(shape, float('nan')) if k in FLOATS else torch.full(shape, -77, dtype=torch.int32)
        out[k], buffers[k] = guarded(fill, float('nan') if k in FLOATS else -77)
    call = lambda: ops.ppo_collect_model(z0, app, params, emb_w, emb_b, gnn, rh, u, H, deep, 2, st.dyn.use_elu, st.dyn.loop_consts(), HW,
                                         DISCOUNT, out=out)
    if not graph:
        call()
    else:
        fresh = {k: ten.clone() for k, ten in out.items()}
        restore = lambda: [ten.copy_(fresh[k]) for k, ten in out.items()]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            call()                                          # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        restore()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            call()
        restore()                                           # (a capture runs nothing)
        g.replay()
    torch.cuda.synchronize()
    return out, buffers


@functools.lru_cache(maxsize=None)
def kernel_run(name):
    """the kernel's collection of the case as host arrays; computed once, read only"""
    from control_harness import margins_intact
    out, buffers = collect(name)
    margins_intact(buffers)
    got = {k: ten.cpu().numpy() for k, ten in out.items()}
    for a in got.values():
        a.setflags(write=False)
    return got


def states_before(name, got):
    """(B, S + 1, N, cl/2 + 2): the state every observation row was taken from -- z0, then the kernel's own z_pred"""
    z0 = start(name)[0].cpu().numpy()
    return np.concatenate([z0[:, None], got['z_pred']], axis=1)
