"""Shared cases of the tests of the model-based PPO arm's collection (tests/test_ppo_model_cpu.py, tests/test_gpu_ppo_model.py): the
seeded shape cases, their policies (ppo_cases.policy), a seeded action-conditioned Stove per object count built the way
tests/test_gpu_env.py builds its model, start states that the model itself rolled out, and the kernel's collection of each case
(computed once per case, never modified)."""
import functools

import numpy as np
import torch

import ppo_cases as P
from stove_amd.rl.collect import uniforms

DEV = 'cuda:0'
HW, DISCOUNT, MIN_MARGIN = 10.0, P.DISCOUNT, P.MIN_MARGIN
# name -> (B, S, N, H, deep, app_dim, debug_nonlinear, seed of the u table).  debug_nonlinear 'relu' is the dynamics' leaky ReLU,
# 'leaky_relu' its ELU (Dynamics.use_elu).  The table is collect.uniforms(B, S, seed); the seed is the first from 4100 on whose smallest
# decision margin in the host forest, on the kernel's own states, is >= 1e-9 (asserted by the GPU tests, no trajectory left out): with
# float32 uniforms a draw violates that with a chance of about 2e-8, so no seed had to be passed over.
CASES = {
    'b1_s1_n1_h32': (1, 1, 1, 32, False, 0, 'relu', 4100),                  # no edges, no appearance
    'b3_s5_n3_h64': (3, 5, 3, 64, False, 3, 'relu', 4100),                  # the workload's kind
    'b3_s5_n3_h64_elu': (3, 5, 3, 64, False, 3, 'leaky_relu', 4100),        # the other activation of the dynamics
    'b3_s5_n4_h40': (3, 5, 4, 40, False, 3, 'relu', 4100),                  # the last wave-per-row count; H no multiple of 32
    'b3_s4_n5_h64_deep': (3, 4, 5, 64, True, 3, 'relu', 4100),              # half-wave rows
    'b5_s6_n6_h128_deep': (5, 6, 6, 128, True, 3, 'relu', 4100),            # the widest; image not staged; B above the wave count
}
KEYS = ('z_pred', 'pred', 'obs', 'actions', 'rewards', 'values', 'logp', 'next_value', 'returns', 'status')
FLOATS = ('z_pred', 'pred', 'obs', 'rewards', 'values', 'logp', 'next_value', 'returns')


def policy(name):
    B, S, N, H, deep = CASES[name][:5]
    return P.policy(N, H, deep)


@functools.lru_cache(maxsize=None)
def model(N, app_dim, nonlinear):
    """an untrained, seeded action-conditioned cl = 32 Stove on N objects (as tests/test_gpu_env.py: _small_model); read only"""
    from test_gpu_dynamics import make_cfg
    from stove_amd.video_prediction.stove import Stove
    assert app_dim in (0, 3)
    state = torch.get_rng_state()
    torch.manual_seed(0)
    st = Stove(make_cfg(num_obj=N, action_conditioned=True, action_space=9, debug_core_appearance=app_dim > 0, debug_appearance_dim=3,
                        debug_nonlinear=nonlinear, debug_match_objects='3_only' if N == 3 else 'greedy')).to(DEV)
    torch.set_rng_state(state)
    assert st.c.cl == 32 and st.c.action_conditioned and st.dyn.use_elu == (nonlinear == 'leaky_relu')
    for p in st.parameters():
        p.requires_grad_(False)
    return st


def case_model(name):
    return model(CASES[name][2], CASES[name][5], CASES[name][6])


def weights(st):
    """what stove_ppo_collect_model reads of the model: embedding, GNN image, reward-head block (stove_plan_expand's set)"""
    from stove_amd.mcts.mcts_stove import BatchedMCTSHandler
    with torch.no_grad():
        return BatchedMCTSHandler._fused_weights(st)


@functools.lru_cache(maxsize=None)
def start(name):
    """-> (z0 (B, N, 18), app (B, N, app_dim) or None) on the device: seeded states (scales 0.1, positions in +-0.7, velocities in +-0.1,
    latents in +-0.5) rolled two steps through the model under seeded actions, so that they lie where the model operates; read only"""
    B, S, N, H, deep, app_dim = CASES[name][:6]
    st = case_model(name)
    rs = np.random.RandomState(5200 + 10 * N + B)
    z = np.concatenate([np.full((B, N, 2), 0.1), rs.uniform(-0.7, 0.7, (B, N, 2)), rs.uniform(-0.1, 0.1, (B, N, 2)),
                        rs.uniform(-0.5, 0.5, (B, N, 12))], axis=2).astype(np.float32)
    app = torch.from_numpy(rs.uniform(0, 1, (B, N, app_dim)).astype(np.float32)).to(DEV) if app_dim else None
    acts = torch.nn.functional.one_hot(torch.from_numpy(rs.randint(0, 9, (B, 2))), 9).float().to(DEV)
    with torch.no_grad():
        z0 = st.rollout(torch.from_numpy(z).to(DEV), 2, actions=acts, appearance=app)[0][:, -1].contiguous()
    assert bool(torch.isfinite(z0).all())
    return z0, app


@functools.lru_cache(maxsize=None)
def table(name):
    """u (B, S) float32 in [0, 1); read only"""
    B, S = CASES[name][:2]
    u = uniforms(B, S, CASES[name][7])
    u.setflags(write=False)
    return u


def shapes(name):
    B, S, N = CASES[name][:3]
    return {'z_pred': (B, S, N, 18), 'pred': (B, S, N, 32), 'obs': (B, S + 1, 4 * N), 'actions': (B, S), 'rewards': (B, S), 'values': (B, S),
            'logp': (B, S), 'next_value': (B,), 'returns': (B, S), 'status': (B,)}


def collect(name, z0=None, graph=False):
    """ops.ppo_collect_model on guarded device copies of the case's inputs; the outputs pre-filled with NaN / -77
    -> (out dict of device tensors, every guarded buffer)"""
    from control_harness import guarded
    from stove_amd import ops
    B, S, N, H, deep, app_dim = CASES[name][:6]
    st = case_model(name)
    z_start, app = start(name)
    buffers, out = {}, {}
    z0, buffers['z0'] = guarded((z_start if z0 is None else z0).cpu(), float('nan'))
    if app is not None:
        app, buffers['app'] = guarded(app.cpu(), float('nan'))
    params, buffers['params'] = guarded(policy(name).flat_params(), float('nan'))
    u, buffers['u'] = guarded(torch.from_numpy(np.array(table(name))), float('nan'))
    emb_w, emb_b, gnn, rh = weights(st)
    for k, shape in shapes(name).items():
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
    """(B, S + 1, N, 18): the state every observation row was taken from -- z0, then the kernel's own z_pred"""
    z0 = start(name)[0].cpu().numpy()
    return np.concatenate([z0[:, None], got['z_pred']], axis=1)
