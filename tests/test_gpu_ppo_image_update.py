"""GPU tests of the image policy's PPO update on the device (stove_ppo_update_images, csrc/ppo_image_update.hip;
ops.ppo_update_images; PPOAgent(fused_images=True)): the kernels against the reference's recorded float64 updates
(tests/golden/g27_ppo_image_update.npz) and, on the six seeded cases, against this project's float64 torch update on the CPU.  The bar
is 4 x max(gap, u) per case and quantity (ppo_image_update_cases says what gap and u are), never taken from the kernels.  Every
decision of the float64 runs has a margin >= 1e-5, so both sides decide alike.  Nothing here reads the reference.  (All fail before the
feature: the symbol, the op, the keyword and update_windows do not exist.)"""
import ctypes

import numpy as np
import pytest
import torch

import control_harness
import ppo_image_cases as P
import ppo_image_update_cases as U
from ppo_update_cases import HYPER

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
POISON = -77.0
BITS = ('image', 'm', 'v', 'losses', 'gnorm')


def _device_update(shape, k, batch, max_steps=None, frames=None, S=None, want_grad=False):
    """ops.ppo_update_images on device copies of the kernel inputs (frames given: the windows are read from them instead of k['obs']),
    the outputs poisoned beforehand -> dict of numpy image, m, v, step, losses, gnorm, status [, grad]"""
    from stove_amd import ops
    F, H, deep = shape
    E, n = k['perm'].shape
    M = batch['M']
    t = {key: torch.from_numpy(a).to(DEV) for key, a in k.items()}
    m, v, step = torch.zeros_like(t['image']), torch.zeros_like(t['image']), torch.zeros(1, dtype=torch.int32, device=DEV)
    out = {'losses': torch.full((E * M, 3), POISON, device=DEV), 'gnorm': torch.full((E * M,), POISON, device=DEV),
           'status': torch.full((2,), -77, dtype=torch.int32, device=DEV)}
    if want_grad:
        out['grad'] = torch.full_like(t['image'], POISON)
    obs = t['obs'] if frames is None else torch.from_numpy(frames).to(DEV)
    out = ops.ppo_update_images(t['image'], m, v, step, obs, t['actions'], t['returns'], t['values'], t['logp'], t['adv'], t['perm'], M, F, H, deep,
                                *(batch[h] for h in HYPER), True, max_steps, S, out)
    res = {key: ten.cpu().numpy() for key, ten in out.items()}
    res.update(image=t['image'].cpu().numpy(), m=m.cpu().numpy(), v=v.cpu().numpy(), step=int(step.cpu()))
    return res


def _same_bits(a, b, keys=BITS):
    for key in keys:
        assert np.array_equal(a[key].view(np.int32), b[key].view(np.int32)), key
    assert a['status'].tolist() == b['status'].tolist() and a['step'] == b['step']


def _case_inputs(name):
    c = U.case(name)
    return c, U.kernel_inputs(c['shape'], c['start'], c['batch'])


# ------------------------------------------------------------------------------------------------ the bars
@pytest.mark.parametrize('c', U.GOLDEN_CASES)
def test_kernels_hold_the_recorded_updates_to_the_bar(c):
    """the four g27 cases: parameters after the update per state_dict key, the losses of every step and the gradient norms"""
    G, batch, shape = U.golden(), U.golden_batch(c), P.GOLDEN_SHAPES[c // 2]
    out = _device_update(shape, U.kernel_inputs(shape, U.golden_start(c), batch), batch)
    assert out['status'].tolist() == [0, 8] and out['step'] == 8
    got = U.distances(shape, out['image'], out['losses'], out['gnorm'], U.golden_after(c), G['c%d_losses' % c], G['c%d_gnorm' % c])
    U.hold_to_the_bar('g27 case %d (kernels)' % c, got, *U.golden_bars(c))


@pytest.mark.parametrize('name', list(U.CASES))
def test_kernels_hold_the_seeded_cases_to_the_bar(name):
    """every collection case as an update case and the 70-row one, against the float64 CPU run of PPOAgent.update"""
    c, k = _case_inputs(name)
    assert c['skipped'] <= 1, 'more than one seed in four had a margin below 1e-5'
    E, M = U.CASES[name][:2]
    out = _device_update(c['shape'], k, c['batch'])
    assert out['status'].tolist() == [0, E * M] and out['step'] == E * M
    r64 = c['r64']
    got = U.distances(c['shape'], out['image'], out['losses'], out['gnorm'], r64['sd'], r64['losses'], r64['gnorm'])
    U.hold_to_the_bar('%s (kernels, seed %d)' % (name, c['seed']), got, c['gap'], c['floor'])


@pytest.mark.parametrize('name', ['b10_s7_n3_f4_h16', 'b2_s2_n6_f4_h512_deep'])
def test_the_gradient_image_of_the_first_step_per_layer(name):
    """max_steps = 1 with `grad`: the unclipped gradient per state_dict key against float64 autograd on step 0's mini-batch, the gap
    from float32 autograd on the same rows (Adam's normalised step would hide a wrong magnitude)"""
    c, k = _case_inputs(name)
    out = _device_update(c['shape'], k, c['batch'], max_steps=1, want_grad=True)
    assert out['status'].tolist() == [0, 1] and (out['grad'] != POISON).all()
    g64, gap, floor = U.first_step_gradients(name)
    got = U.state_of_image(c['shape'], out['grad'])
    U.hold_to_the_bar('%s (gradient of step 0)' % name, {'params': {q: float(np.abs(got[q] - g64[q]).max()) for q in g64}}, {'params': gap},
                      {'params': floor})
    norm = np.sqrt(sum(float((g64[q] ** 2).sum()) for q in g64))
    assert abs(float(out['gnorm'][0]) - norm) <= U.FACTOR * max(c['gap']['gnorm'], c['floor']['gnorm'])


# ------------------------------------------------------------------------------------------------ layouts, determinism, partial runs
def test_frames_and_dense_observations_give_the_same_bits():
    c, k = _case_inputs('b5_s3_n3_f4_h16')
    dense = _device_update(c['shape'], k, c['batch'], want_grad=True)
    windows = _device_update(c['shape'], k, c['batch'], frames=c['frames'], S=c['S'], want_grad=True)
    assert dense['status'].tolist() == [0, 6]
    _same_bits(dense, windows, BITS + ('grad',))


def test_two_calls_agree_bit_for_bit():
    for name in ('b10_s7_n3_f4_h16', 'b9_s2_n2_f2_h33_deep'):
        c, k = _case_inputs(name)
        _same_bits(_device_update(c['shape'], k, c['batch'], want_grad=True), _device_update(c['shape'], k, c['batch'], want_grad=True),
                   BITS + ('grad',))


@pytest.mark.parametrize('k_steps', [0, 2, 6])
def test_max_steps_stops_there(k_steps):
    c, k = _case_inputs('b5_s3_n3_f4_h16')
    out = _device_update(c['shape'], k, c['batch'], max_steps=k_steps)
    whole = _device_update(c['shape'], k, c['batch'])
    assert out['status'].tolist() == [0, k_steps] and out['step'] == k_steps
    assert (out['losses'][k_steps:] == POISON).all() and (out['gnorm'][k_steps:] == POISON).all()
    assert np.array_equal(out['losses'][:k_steps].view(np.int32), whole['losses'][:k_steps].view(np.int32))
    assert np.array_equal(out['gnorm'][:k_steps].view(np.int32), whole['gnorm'][:k_steps].view(np.int32))
    if k_steps == 0:
        assert np.array_equal(out['image'], k['image']) and not out['m'].any() and not out['v'].any()
    if k_steps == 6:
        _same_bits(out, whole)


def test_a_nan_advantage_or_a_bad_index_stops_the_update_at_its_step():
    """a NaN in an input is data: status (3, k), everything bit for bit as a clean call with max_steps = k left it; an action of 9 or an
    index of perm equal to n stops the same way with status 2"""
    c, k = _case_inputs('b5_s3_n3_f4_h16')
    M, mb, step_k = 3, 5, 4
    row = int(k['perm'][step_k // M][(step_k % M) * mb + 2])
    steps_of = [at for at in range(6) if row in k['perm'][at // M][(at % M) * mb:(at % M + 1) * mb]]
    first = steps_of[0]
    clean = _device_update(c['shape'], k, c['batch'], max_steps=first)
    bad = dict(k, adv=k['adv'].copy())
    bad['adv'][row] = np.nan
    out = _device_update(c['shape'], bad, c['batch'])
    assert out['status'].tolist() == [3, first] and out['step'] == first
    _same_bits(dict(out, status=np.array([0, first])), clean)
    act = dict(k, actions=k['actions'].copy())
    act['actions'][row] = 9
    out = _device_update(c['shape'], act, c['batch'])
    assert out['status'].tolist() == [2, first]
    _same_bits(dict(out, status=np.array([0, first])), clean)
    idx = dict(k, perm=k['perm'].copy())
    idx['perm'][0][1] = 15
    out = _device_update(c['shape'], idx, c['batch'])
    assert out['status'].tolist() == [2, 0] and out['step'] == 0
    assert np.array_equal(out['image'], k['image']) and not out['m'].any() and not out['v'].any() and (out['losses'] == POISON).all()


def test_an_empty_call():
    c, k = _case_inputs('b5_s3_n3_f4_h16')
    empty = dict(k, perm=np.zeros((0, 15), dtype=np.int32))
    out = _device_update(c['shape'], empty, c['batch'])
    assert out['status'].tolist() == [0, 0] and out['step'] == 0 and np.array_equal(out['image'], k['image'])


# ------------------------------------------------------------------------------------------------ capture, workspace
def test_a_captured_call_replays_like_eager_calls():
    """(E, M) = (1, 2) on the 70-row case: the capture replayed twice equals two eager calls bit for bit"""
    from stove_amd import ops
    c, k = _case_inputs('b10_s7_n3_f4_h16')
    F, H, deep = c['shape']

    def state():
        t = {key: torch.from_numpy(a).to(DEV) for key, a in k.items()}
        t.update(m=torch.zeros_like(t['image']), v=torch.zeros_like(t['image']), step=torch.zeros(1, dtype=torch.int32, device=DEV))
        t['out'] = {'losses': torch.zeros((2, 3), device=DEV), 'gnorm': torch.zeros(2, device=DEV), 'status': torch.zeros(2, dtype=torch.int32, device=DEV)}
        return t

    def call(t):
        ops.ppo_update_images(t['image'], t['m'], t['v'], t['step'], t['obs'], t['actions'], t['returns'], t['values'], t['logp'], t['adv'], t['perm'],
                              2, F, H, deep, *(c['batch'][h] for h in HYPER), out=t['out'])

    eager, graphed = state(), state()
    call(eager)
    call(eager)
    warm = state()
    call(warm)                                                   # (the workspace of this shape exists before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(graphed)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    for key in ('image', 'm', 'v', 'step'):
        assert torch.equal(eager[key], graphed[key]), key
    for key in ('losses', 'gnorm', 'status'):
        assert torch.equal(eager['out'][key], graphed['out'][key]), key
    assert eager['out']['status'].tolist() == [0, 2] and int(eager['step']) == 4


def test_the_margins_of_the_workspace_and_of_every_output_are_intact():
    """the C entry on guarded buffers: ws of exactly stove_ppo_update_images_ws_bytes bytes, every output and in/out array"""
    from stove_amd import _lib
    from stove_amd.ops import ptr, stream
    lib = _lib.load()
    c, k = _case_inputs('b9_s2_n2_f2_h33_deep')
    F, H, deep = c['shape']
    E, n = k['perm'].shape
    M = c['batch']['M']
    nbytes = int(lib.stove_ppo_update_images_ws_bytes(n, M, F, H, int(deep)))
    assert nbytes > 0 and nbytes % 4 == 0
    nan = float('nan')
    views, bufs = {}, {}
    for key, (values, fill) in {'image': (torch.from_numpy(k['image']), nan), 'm': (torch.zeros(k['image'].size), nan),
                                'v': (torch.zeros(k['image'].size), nan), 'step': (torch.zeros(1, dtype=torch.int32), -77),
                                'losses': (torch.zeros(E * M, 3), nan), 'gnorm': (torch.zeros(E * M), nan), 'grad': (torch.zeros(k['image'].size), nan),
                                'status': (torch.zeros(2, dtype=torch.int32), -77), 'ws': (torch.zeros(nbytes // 4), nan)}.items():
        views[key], bufs[key] = control_harness.guarded(values, fill, device=DEV)
    t = {key: torch.from_numpy(k[key]).to(DEV) for key in ('obs', 'actions', 'returns', 'values', 'logp', 'adv', 'perm')}
    b = c['batch']
    with torch.cuda.device(DEV):
        code = lib.stove_ppo_update_images(ptr(views['image']), ptr(views['m']), ptr(views['v']), ptr(views['step']), ptr(t['obs']), ptr(t['actions']),
                                           ptr(t['returns']), ptr(t['values']), ptr(t['logp']), ptr(t['adv']), ptr(t['perm']), ptr(views['losses']),
                                           ptr(views['gnorm']), ptr(views['grad']), ptr(views['status']), ptr(views['ws']), n, 1, 3072 * F, E, M,
                                           E * M, F, H, int(deep), *(ctypes.c_float(b[h]) for h in HYPER), 1, stream())
    assert code == 0
    torch.cuda.synchronize()
    assert views['status'].tolist() == [0, E * M] and int(views['step']) == E * M
    control_harness.margins_intact(bufs)
    ref = _device_update(c['shape'], k, b, want_grad=True)
    for key in ('image', 'm', 'v', 'losses', 'gnorm', 'grad'):
        assert np.array_equal(views[key].cpu().numpy().view(np.int32).reshape(-1), ref[key].view(np.int32).reshape(-1)), key


# ------------------------------------------------------------------------------------------------ the agent and the runner
def _torch_state(seed, fn):
    state = torch.get_rng_state()
    torch.manual_seed(seed)
    try:
        return fn()
    finally:
        torch.set_rng_state(state)


@pytest.mark.parametrize('how', ['update_windows', 'update'])
def test_agent_follows_the_float64_torch_agent_under_the_same_seed(how):
    from stove_amd.rl.agents import PPOAgent
    name = 'b5_s3_n3_f4_h16'
    c = U.case(name)
    b, shape = c['batch'], c['shape']
    r64 = U.traced_update(U.policy_of(shape, c['start'], torch.float64), {k: v for k, v in b.items() if k != 'perm'}, torch.float64, seed=7)
    r32 = U.traced_update(U.policy_of(shape, c['start']), b, torch.float32, perm=r64['perm'])
    assert min(r64['margins'].values()) >= U.MIN_MARGIN, r64['margins']
    policy = U.policy_of(shape, c['start']).to(DEV)
    agent = PPOAgent(policy, b['clip'], b['E'], b['M'], b['value_coef'], b['entropy_coef'], lr=b['lr'], eps=b['eps'], max_grad_norm=b['max_grad_norm'],
                     fused_images=True)
    col = lambda key: torch.from_numpy(np.asarray(b[key], dtype=np.float32)).reshape(-1, 1).to(DEV)
    acts = torch.from_numpy(b['actions']).reshape(-1, 1).to(DEV)
    if how == 'update':
        returned = _torch_state(7, lambda: agent.update(torch.from_numpy(b['obs']).to(DEV), acts, col('returns'), col('values'), col('logp'), col('adv')))
    else:
        returned = _torch_state(7, lambda: agent.update_windows(torch.from_numpy(c['frames']).to(DEV), c['S'], acts, col('returns'), col('values'),
                                                                  col('logp'), col('adv')))
    gap, floor = U.gap_of(shape, r64, r32), U.floor_of(shape, r64['sd'], r64['losses'], r64['gnorm'])
    got = {k: float(np.abs(t.double().cpu().numpy() - r64['sd'][k]).max()) for k, t in policy.state_dict().items() if k in gap['params']}
    U.hold_to_the_bar('agent.%s' % how, {'params': got}, {'params': gap['params']}, {'params': floor['params']})
    for q, value, want in zip(U.STEP_QUANTITIES[:3], returned, r64['returned']):
        assert abs(value - want) <= U.FACTOR * max(gap[q], floor[q]), q
    assert int(agent._moments[2]) == b['E'] * b['M']
    nan = col('adv')
    nan[3] = float('nan')
    with pytest.raises(RuntimeError, match='status 3'):
        agent.update(torch.from_numpy(b['obs']).to(DEV), acts, col('returns'), col('values'), col('logp'), nan)


def test_runner_with_a_fused_images_agent_runs_batches_on_the_frames():
    """PPORunner.run_batch on a device BatchedAvoidance, B = 4, S = 6, (E, M) = (2, 3): two batches, finite losses, a changed policy"""
    from stove_amd.envs import envs
    from stove_amd.rl.agents import PPOAgent
    from stove_amd.rl.runners import PPORunner
    env = envs.BillardsEnv(n=3, granularity=2, seed=5)
    task = envs.AvoidanceTask(env, num_stacked=4, action_force=.3)
    policy = U.policy_of((4, 16, False), P.policy(4, 16, False).state_dict())
    before = {k: t.clone() for k, t in policy.state_dict().items()}
    agent = PPOAgent(policy, .1, 2, 3, .5, .01, lr=2e-4, eps=1e-5, max_grad_norm=40, fused_images=True)
    runner = PPORunner(env, task, None, DEV, agent, policy, num_steps=6, batch_size=4, discount=P.DISCOUNT)
    assert runner.fused_serves_images()
    runner.stacked = None          # (no stacked observation is built on this path)
    for batch in range(2):
        u = np.random.RandomState(3 + batch).random_sample((4, 6)).astype(np.float32)
        out = _torch_state(1 + batch, lambda: runner.run_batch(u=u))
        assert all(np.isfinite(l) for l in out['losses']) and tuple(out['frames'].shape) == (4, 10, 3, 32, 32)
    del runner.stacked
    assert int(agent._moments[2]) == 12 and runner.batch_counter == 2
    moved = max(float((t.cpu() - before[k]).abs().max()) for k, t in policy.state_dict().items() if 'in_between' not in k)
    assert moved > 1e-4, moved
