"""GPU tests of the batched avoidance environments (stove_env_step, csrc/env.hip; ops.env_step; BatchedAvoidance on a device) and of
closed-loop planning with them (stove_amd/mcts/play.py): the kernel against the numpy class BatchedAvoidance(device=None) -- the same
text, csrc/env_step.h, is held to that class on the CPU by tests/test_env_batched_cpu.py -- bit for bit in x, v and collisions, frames
to one float32 ulp (2^-23: exp is a library call on either side, everything else is the same IEEE operations before one rounding).
The trajectories are those of tests/env_cases.py, stepped free-running for 24 steps: bitwise equality leaves no drift to allow for."""

import numpy as np
import pytest
import torch

import env_cases as C
from control_harness import guarded, margins_intact

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ULP32 = 2.0 ** -23
INVALID = 1          # hipErrorInvalidValue


def _batch(name, M, res, use_colors):
    """a host BatchedAvoidance of M environments: row e is environment e % M0 of case `name` -> (batch, rows)"""
    from stove_amd.envs.batched import BatchedAvoidance
    tasks = C.start(name).tasks()
    rows = np.arange(M) % len(tasks)
    b = BatchedAvoidance.from_tasks([tasks[i] for i in rows])
    b.res, b.use_colors = res, use_colors
    return b, rows


def _device_state(b, render=True):
    """guarded device copies of a host batch's arrays and of the outputs"""
    t, buffers = {}, {}
    for k in ('x', 'v', 'r', 'm'):
        t[k], buffers[k] = guarded(torch.from_numpy(getattr(b, k).copy()), float('nan'))
    t['collisions'], buffers['collisions'] = guarded(torch.full((b.M,), -7, dtype=torch.int32), -77)
    t['status'], buffers['status'] = guarded(torch.full((b.M,), -7, dtype=torch.int32), -77)
    t['frames'] = None
    if render:
        t['frames'], buffers['frames'] = guarded(torch.full((b.M, 3, b.res, b.res), float('nan')), float('nan'))
    return t, buffers


def _step(b, t, action):
    from stove_amd import ops
    return ops.env_step(t['x'], t['v'], t['r'], t['m'], action, b.granularity, b.res, b.hw, b.t, b.friction, b.action_force,
                        use_colors=b.use_colors, drift=b.drift, render=t['frames'] is not None, out=(t['frames'], t['collisions'], t['status']))


def _same_bits(got, want):
    return np.array_equal(np.ascontiguousarray(got).view(np.int64), np.ascontiguousarray(want).view(np.int64))


# ------------------------------------------------------------------------------------------------ 5. kernel = numpy class
# M = 1, 4 and 65 (past one wave of environments); N = 1, 3, 6; res 32 and 50 (2500 pixels: no multiple of the 256 lanes); colours on
# and off; granularity 5 and 50; action = None; frames = None; friction and drift
@pytest.mark.parametrize('name,M,res,use_colors,render', [
    ('n1', 1, 32, False, True), ('n3', 4, 32, True, True), ('n3', 65, 50, False, True), ('n6', 4, 50, True, True), ('n6', 65, 32, False, True),
    ('n2', 1, 50, True, True), ('n3_g50', 4, 32, True, True), ('n3_none', 4, 32, True, True), ('n3', 4, 32, True, False),
    ('n3_fric', 4, 32, False, True), ('n3_drift', 4, 32, True, True)])
def test_kernel_equals_the_numpy_class(name, M, res, use_colors, render):
    host = C.host_run(name)
    acts = C.actions(name)
    b, rows = _batch(name, M, res, use_colors)
    t, buffers = _device_state(b, render)
    assert (b.n, b.granularity) == C.CASES[name][:2]
    worst = 0.0
    for s in range(C.STEPS):
        action = None if acts is None else torch.from_numpy(acts[s, rows].astype(np.int32)).to(DEV)
        frames, collisions, status = _step(b, t, action)
        assert (frames is None) == (not render)
        x, v = t['x'].cpu().numpy(), t['v'].cpu().numpy()
        assert not status.cpu().numpy().any(), (name, s)
        assert _same_bits(x, host['x'][s][rows]) and _same_bits(v, host['v'][s][rows]), (name, s)
        assert np.array_equal(collisions.cpu().numpy(), host['collisions'][s][rows]), (name, s)
        if render and s % 4 == 3:
            b.x = host['x'][s][rows]
            want = b.frames()
            got = frames.cpu().numpy()
            assert got.shape == want.shape == (M, 3, res, res)
            worst = max(worst, float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()))
    print(f'env_step {name} M={M} res={res} colours={use_colors}: frames against the numpy class {worst:.3g} (bar {ULP32:.3g})')
    assert worst <= ULP32
    if render:
        assert float(got.max()) > 0.99 and float(got.min()) == 0.0
    margins_intact(buffers)


# ------------------------------------------------------------------------------------------------ 6. status, refusals
@pytest.mark.parametrize('bad', [9, -1])
def test_status_two(bad):
    """environment 1 of 3 gets an action index outside [0, 9): status [0, 2, 0], its x, v, collisions entry and frame untouched, the
    twins 0 and 2 as in a clean run"""
    from stove_amd.envs.batched import BatchedAvoidance
    b = BatchedAvoidance([0, 1, 0])
    t, buffers = _device_state(b)
    clean, _ = _device_state(b)
    _step(b, clean, torch.tensor([1, 3, 1], dtype=torch.int32, device=DEV))
    _, _, status = _step(b, t, torch.tensor([1, bad, 1], dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert status.tolist() == [0, 2, 0] and clean['status'].tolist() == [0, 0, 0]
    assert _same_bits(t['x'][1].cpu().numpy(), b.x[1]) and _same_bits(t['v'][1].cpu().numpy(), b.v[1])
    assert int(t['collisions'][1]) == -7 and bool(torch.isnan(t['frames'][1]).all())
    for k in ('x', 'v'):
        assert torch.equal(t[k][[0, 2]].view(torch.int64), clean[k][[0, 2]].view(torch.int64)), k
        assert torch.equal(t[k][0].view(torch.int64), t[k][2].view(torch.int64)), k
    assert torch.equal(t['frames'][[0, 2]].view(torch.int32), clean['frames'][[0, 2]].view(torch.int32))
    assert torch.equal(t['collisions'][[0, 2]], clean['collisions'][[0, 2]])
    assert not _same_bits(t['x'][0].cpu().numpy(), b.x[0])
    margins_intact(buffers)
    # the class: the same through BatchedAvoidance on the device and on the host
    dev, host = BatchedAvoidance([0, 1, 0], device=DEV), BatchedAvoidance([0, 1, 0])
    dev.step([1, bad, 1])
    host.step([1, bad, 1])
    assert dev.status.tolist() == host.status.tolist() == [0, 2, 0]
    assert _same_bits(dev.x.cpu().numpy(), host.x) and _same_bits(dev.state().cpu().numpy(), host.state())


def test_host_visible_refusals_launch_nothing():
    from stove_amd import _lib
    from stove_amd.envs.batched import BatchedAvoidance
    lib = _lib.load()
    b = BatchedAvoidance([0, 1, 0])
    t, buffers = _device_state(b)
    before = {k: v.clone() for k, v in buffers.items()}
    p = {k: (v.data_ptr() if v is not None else None) for k, v in t.items()}

    def call(M=3, N=3, gran=5, res=32, **null):
        a = dict(p, action=None, **{k: None for k in null})
        return lib.stove_env_step(a['x'], a['v'], a['r'], a['m'], a['action'], a['collisions'], a['status'], a['frames'], M, N, gran, res, 1, 0,
                                  10.0, 1.0, 0.0, 0.6, _lib.stream())
    for k in ('x', 'v', 'r', 'm', 'collisions', 'status'):
        assert call(**{k: True}) == INVALID, k
    assert call(M=-1) == INVALID and call(N=0) == INVALID and call(N=7) == INVALID and call(gran=0) == INVALID and call(res=0) == INVALID
    assert call(M=0) == 0
    torch.cuda.synchronize()
    for k in buffers:
        assert torch.equal(buffers[k].view(torch.int32), before[k].view(torch.int32)), k
    assert call() == 0                                    # and the valid call still runs
    torch.cuda.synchronize()
    assert t['status'].tolist() == [0, 0, 0]
    margins_intact(buffers)


# ------------------------------------------------------------------------------------------------ 7. graph capture
def test_captured_step_replays_bit_for_bit():
    b, rows = _batch('n3', 4, 32, True)
    action = torch.from_numpy(C.actions('n3')[0, rows].astype(np.int32)).to(DEV)
    eager, _ = _device_state(b)
    for _ in range(3):
        _step(b, eager, action)
    t, buffers = _device_state(b)
    start = {k: t[k].clone() for k in ('x', 'v')}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _step(b, t, action)                              # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for k in ('x', 'v'):
        t[k].copy_(start[k])
    t['frames'].fill_(float('nan'))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _step(b, t, action)
    for k in ('x', 'v'):
        t[k].copy_(start[k])                             # (a capture runs nothing)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    for k in ('x', 'v'):
        assert torch.equal(t[k].view(torch.int64), eager[k].view(torch.int64)), k
    assert torch.equal(t['frames'].view(torch.int32), eager['frames'].view(torch.int32))
    assert torch.equal(t['collisions'], eager['collisions']) and t['status'].tolist() == [0] * 4
    host, _ = _batch('n3', 4, 32, True)
    for _ in range(3):
        host.step(C.actions('n3')[0, rows])
    assert _same_bits(t['x'].cpu().numpy(), host.x) and _same_bits(t['v'].cpu().numpy(), host.v)
    margins_intact(buffers)


# ------------------------------------------------------------------------------------------------ 8. play
def _small_model():
    from test_gpu_dynamics import make_cfg
    from test_gpu_plan import CFG
    from stove_amd.video_prediction.stove import Stove
    torch.manual_seed(0)
    model = Stove(make_cfg(**CFG)).to(DEV)
    assert model.c.cl == 32 and model.c.action_conditioned
    return model


@pytest.fixture(scope='module')
def model():
    return _small_model()


@pytest.mark.parametrize('device_trees', [False, True])
def test_play_with_device_environments(model, device_trees, monkeypatch):
    """an untrained action-conditioned model, M = 3, run_len 3, 6 expansions, depth 2: the returned states and rewards equal, bit for
    bit, a host BatchedAvoidance replaying the returned actions, and the frame ring handed to the planner at each step is the
    host-rendered ring of that replay to 2^-23.  (Which actions an episode chooses is not compared across environment paths.)"""
    from stove_amd.envs.batched import BatchedAvoidance
    from stove_amd.mcts import play as P
    seen = []
    planner = P.plan_on_frames

    def recording(x, mdl, actions, *a, **k):
        assert x.is_cuda and actions.is_cuda and x.dtype == torch.float32
        seen.append((x.clone(), actions.clone()))
        return planner(x, mdl, actions, *a, **k)
    monkeypatch.setattr(P, 'plan_on_frames', recording)
    np.random.seed(11)
    envs = BatchedAvoidance([0, 3, 4], device=DEV)
    got = P.play(model, envs, run_len=3, mcts_steps=6, max_rollout_depth=2, device_trees=device_trees, keep_frames=True)
    assert got['actions'].shape == (3, 3) and got['actions'].dtype == np.int64 and ((got['actions'] >= 0) & (got['actions'] < 9)).all()
    assert got['states'].shape == (3, 3, 3, 4) and got['rewards'].shape == (3, 3) and got['frames'].shape == (3, 3, 3, 32, 32)
    host = BatchedAvoidance([0, 3, 4])
    rings = P.warm_up(host)
    assert len(seen) == 3
    for s in range(3):
        x, a = rings.tensors()
        assert float((seen[s][0].cpu().double() - x.double()).abs().max()) <= ULP32, s
        assert torch.equal(seen[s][1].cpu(), a), s
        reward, state = rings.step(got['actions'][s])
        assert _same_bits(got['states'][s], state) and np.array_equal(got['rewards'][s], reward), s
        assert float(np.abs(got['frames'][s].astype(np.float64) - host.frames()).max()) <= ULP32
    assert _same_bits(envs.state().cpu().numpy(), host.state())


def test_play_on_a_list_is_the_hand_composed_loop(model):
    from stove_amd.mcts.mcts_stove import initialize_img, run_mcts_model, update_buffer
    from stove_amd.mcts.play import play
    mk = lambda: [t for i, t in enumerate(C.make_tasks('n3')) if i in (0, 1, 2)]
    np.random.seed(12)
    got = play(model, mk(), run_len=3, mcts_steps=6, max_rollout_depth=2)
    np.random.seed(12)
    tasks = mk()
    img, actions = initialize_img(tasks, steps=8, res=32)
    for s in range(3):
        nxt = run_mcts_model(img, model, actions, num_parallel_envs=3, mcts_steps=6, max_rollout_depth=2)
        res = [t.step(nxt[j]) for j, t in enumerate(tasks)]
        img, actions = update_buffer(img, np.stack([r[0] for r in res]), actions, nxt)
        assert got['actions'][s].tolist() == nxt, s
        assert np.array_equal(got['states'][s], np.stack([r[1] for r in res])) and got['rewards'][s].tolist() == [r[2] for r in res], s


# ------------------------------------------------------------------------------------------------ 9. plan_on_frames
@pytest.mark.parametrize('device_trees', [False, True])
def test_plan_on_frames_is_plan_on_model(model, device_trees):
    from stove_amd.mcts.mcts_stove import encode_img, initialize_img, plan_on_frames, plan_on_model
    img, actions = initialize_img(C.make_tasks('n3')[:3], steps=8, res=32)
    np.random.seed(1)
    want = plan_on_model(img, model, actions, num_parallel_envs=3, mcts_steps=8, max_rollout_depth=3, device_trees=device_trees)
    np.random.seed(1)
    got = plan_on_frames(encode_img(img).to(DEV), model, actions, num_parallel_envs=3, mcts_steps=8, max_rollout_depth=3, device_trees=device_trees)
    assert got == want and all(isinstance(a, int) and 0 <= a < 9 for a in got)
