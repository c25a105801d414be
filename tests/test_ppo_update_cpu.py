"""CPU-side checks (-m "not gpu") of the one-launch PPO update: the fixture g25 (the reference's PPOAgent.update, step by step) is
sound and this project's float64 torch update reproduces it; the text the kernel runs, stove_amd/csrc/ppo_update.h, compiled host-only
under sanitizers with contraction off (tests/abi/ppo_update_driver.cpp), held to the bar on the six recorded cases and on the edge
shapes; Policy.load_flat_params; the entry point refusing host-visible nonsense; the refusals that need no device.  (The header, the
symbol, load_flat_params and the `fused` keyword do not exist before the feature.)"""
import ctypes

import numpy as np
import pytest
import torch

import control_harness
import ppo_update_cases as U



# ------------------------------------------------------------------------------------------------ 1. the fixture
@pytest.mark.parametrize('c', U.CASES)
def test_torch_update_reproduces_the_recorded_update_in_float64(c):
    """parameters, per-step losses and gradient norms to 1e-10 of each tensor's largest entry; the recorded permutations are what
    torch.randperm draws under the recorded seed"""
    G, batch = U.golden(), U.golden_batch(c)
    close = lambda got, want: np.abs(np.asarray(got) - want).max() <= 1e-10 * max(np.abs(want).max(), 1e-300)
    batch['E'] = int(G['EM'][0])
    run = U.traced_update(U.golden_start(c, torch.float64), batch, torch.float64, seed=0)
    assert np.array_equal(run['perm'], batch['perm'])
    assert close(run['losses'], G['c%d_losses' % c]) and close(run['gnorm'], G['c%d_gnorm' % c]) and close(run['returned'], G['c%d_returned' % c])
    after, moved = U.golden_after(c), 0.0
    start = U.golden_start(c, torch.float64).state_dict()
    for key, want in after.items():
        assert close(run['sd'][key], want), key
        moved = max(moved, float(np.abs(want - start[key].numpy()).max()))
    assert moved > 1e-4                                         # (the update did something)


def test_fixture_margins_and_clipping():
    gaps, G = U.gaps(), U.golden()
    assert sorted(gaps) == ['case%d' % c for c in U.CASES]
    for c in U.CASES:
        g = gaps['case%d' % c]
        assert g['shape'] == list(U.GOLDEN_SHAPES[c // 2]) and g['kind'] == ('plain', 'clip')[c % 2]
        assert min(g['margins'].values()) >= U.MIN_MARGIN, g['margins']
        norms, bound = G['c%d_gnorm' % c], float(G['c%d_hyper' % c][5])
        assert bound == g['max_grad_norm'] and norms.shape == (8,)
        assert (norms > bound).all() if c % 2 else (norms < bound).all()
        assert all(g['gap'][q] > 0 for q in U.QUANTITIES)
        print('case %d: margins %s, gap %s' % (c, g['margins'], g['gap']))


# ------------------------------------------------------------------------------------------------ 2. the header on the CPU
@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    return control_harness.build_driver(tmp_path_factory, 'ppo_update_driver')


def _drive(exe, tmp_path, shape, k, batch, max_steps=None, clipped=True, step=0):
    """one whole update through the driver -> dict image, m, v, step, status, done, losses (E M, 3), gnorm (E M,)"""
    N, H, deep = shape
    E, n = k['perm'].shape
    M = batch['M']
    zeros, P = np.zeros_like(k['image']), k['image'].size
    outputs = [('image', (P,), np.float32), ('m', (P,), np.float32), ('v', (P,), np.float32), ('tail', (3,), np.int32),
               ('losses', (E * M, 3), np.float32), ('gnorm', (E * M,), np.float32)]
    out = control_harness.run_driver(exe, tmp_path, [n, E, M, E * M if max_steps is None else max_steps, N, H, int(deep), int(clipped), step],
                                     np.array([batch[h] for h in U.HYPER], dtype=np.float32),
                                     [k['image'], zeros, zeros, k['obs'], k['actions'], k['returns'], k['values'], k['logp'], k['adv'], k['perm']], outputs)
    out['step'], out['status'], out['done'] = (int(x) for x in out.pop('tail'))
    return out


@pytest.mark.parametrize('c', U.CASES)
def test_header_holds_the_recorded_updates_to_the_bar(driver, tmp_path, c):
    """Parameters, the three losses of every step and the gradient norms against the reference's float64 update; the bar is 4 x the
    reference's own float32-to-float64 gap of that case and quantity (g25_reference_fp32_gap.json).  Measured on the CPU (the kernel
    runs the same text; tests/test_gpu_ppo_update.py prints its own): parameters 1.0 .. 1.1 x the gap, the losses 0.3 .. 2.1 x (the
    value loss of case 1), the norms 0.4 .. 0.7 x."""
    G, batch, shape = U.golden(), U.golden_batch(c), U.GOLDEN_SHAPES[c // 2]
    out = _drive(driver, tmp_path, shape, U.kernel_inputs(U.golden_start(c), batch), batch)
    assert (out['status'], out['done'], out['step']) == (0, 8, 8)
    got = U.distances(shape, out['image'], out['losses'], out['gnorm'], U.golden_after(c), G['c%d_losses' % c], G['c%d_gnorm' % c])
    U.hold_to_the_bar('case %d (header)' % c, got, U.gaps()['case%d' % c]['gap'])


@pytest.mark.parametrize('name', list(U.EDGES))
def test_header_holds_the_edge_shapes_to_the_bar(driver, tmp_path, name):
    """against this project's float64 torch update; the gap is its float32 run on the same permutations"""
    shape, start, batch, r64, gap, seed, skipped = U.edge(name)
    assert skipped <= 1, 'more than one seed in four had a margin below 1e-5'
    E, M = U.EDGES[name][4:6]
    out = _drive(driver, tmp_path, shape, U.kernel_inputs(U.policy_of(shape, start), batch), batch)
    assert (out['status'], out['done'], out['step']) == (0, E * M, E * M)
    U.hold_to_the_bar('%s (header, seed %d)' % (name, seed), U.distances(shape, out['image'], out['losses'], out['gnorm'], r64['sd'], r64['losses'],
                                                                       r64['gnorm']), gap)


def test_header_unclipped_value_loss_and_a_later_step_count(driver, tmp_path):
    """use_clipped_value_loss=False in the header: one step against torch autograd on 0.5 (v - R)^2 in float64, to the clipped case's
    bar; and an update that starts at step count 5 takes Adam's bias corrections from there (a different result than from 0)."""
    c, shape = 0, U.GOLDEN_SHAPES[0]
    batch, gap = U.golden_batch(c), U.gaps()['case0']['gap']
    k = U.kernel_inputs(U.golden_start(c), batch)
    out = _drive(driver, tmp_path, shape, k, batch, max_steps=1, clipped=False)
    policy = U.golden_start(c, torch.float64)
    rows = torch.from_numpy(batch['perm'][0][:16])
    col = lambda key: torch.from_numpy(batch[key]).double().reshape(-1, 1)[rows]
    value, logp, entropy = policy.evaluate_actions(torch.from_numpy(batch['obs']).double()[rows], torch.from_numpy(batch['actions']).reshape(-1, 1)[rows])
    ratio = torch.exp(logp - col('logp'))
    action_loss = -torch.min(ratio * col('adv'), torch.clamp(ratio, .9, 1.1) * col('adv')).mean()
    value_loss = 0.5 * (value - col('returns')).pow(2).mean()
    optim = torch.optim.Adam(policy.parameters(), lr=batch['lr'], eps=batch['eps'])
    (value_loss * .5 + action_loss - entropy * .01).backward()
    norm = float(torch.nn.utils.clip_grad_norm_(policy.parameters(), 40.))
    optim.step()
    want = {key: t.detach().numpy() for key, t in policy.state_dict().items()}
    got = U.distances(shape, out['image'], out['losses'][:1], out['gnorm'][:1], want, np.array([[value_loss.item(), action_loss.item(), entropy.item()]]),
                      np.array([norm]))
    U.hold_to_the_bar('unclipped value loss, one step', got, gap)
    clipped = _drive(driver, tmp_path, shape, k, batch, max_steps=1)
    assert abs(float(clipped['losses'][0, 0]) - value_loss.item()) > 1e-4          # (the two forms differ on this batch)
    later = _drive(driver, tmp_path, shape, k, batch, max_steps=1, step=5)
    assert later['step'] == 6 and not np.array_equal(later['image'], clipped['image']) and np.array_equal(later['losses'], clipped['losses'])


def test_validation_and_status_under_sanitizers(driver):
    """stove_ppo_update's host-side argument check (csrc/validate.h: ppo_update) through the driver: every documented bad argument
    returns hipErrorInvalidValue, empty calls are accepted, nothing is dereferenced.  Status: a NaN advantage in a row of step k gives
    (3, k) with params, m, v, step, losses and gnorm bit for bit those of a clean run of max_steps = k; an index of perm or an action
    out of range gives (2, k) likewise; the indices an epoch drops are never read."""
    control_harness.run_modes(driver, ['validate', 'status'])


# ------------------------------------------------------------------------------------------------ 3. the image round trip
@pytest.mark.parametrize('deep', [False, True])
@pytest.mark.parametrize('H', [32, 40, 128])
def test_load_flat_params_inverts_flat_params(H, deep):
    from stove_amd.rl.rl_model import Policy
    state = torch.get_rng_state()
    torch.manual_seed(3 + H)
    p = Policy(12, 9, hidden_size=H, base='control', use_deep_layers=deep)
    q = Policy(12, 9, hidden_size=H, base='control', use_deep_layers=deep)
    torch.set_rng_state(state)
    before = {k: t.clone() for k, t in p.state_dict().items()}
    image = p.flat_params()
    p.load_flat_params(image)
    for k, t in p.state_dict().items():
        assert torch.equal(t.view(torch.int32), before[k].view(torch.int32)), k
    q.load_flat_params(image)
    for k, t in q.state_dict().items():
        if deep or 'in_between' not in k:                        # (a shallow image does not hold the unused layers)
            assert torch.equal(t, before[k]), k
    assert torch.equal(q.flat_params(), image)
    assert all(t.requires_grad for t in q.parameters())
    with pytest.raises(ValueError, match='load_flat_params'):
        q.load_flat_params(image[:-1])
    with pytest.raises(ValueError, match='load_flat_params'):
        Policy((32, 32, 12), 9, hidden_size=512).load_flat_params(image)


# ------------------------------------------------------------------------------------------------ 4. bookkeeping
def test_ppo_update_refuses_host_visible_nonsense():
    from stove_amd import _lib, build, ops
    build.build_library()
    fn = _lib.load().stove_ppo_update
    # host-visible nonsense is refused before anything touches a device (there may be none): hipErrorInvalidValue == 1
    Pv = ctypes.c_void_p
    good = ctypes.create_string_buffer(64)
    addr = ctypes.addressof(good)
    call = lambda p=addr, n=64, E=2, M=4, steps=8, N=3, H=64: fn(Pv(p), *([Pv(addr)] * 13), n, E, M, steps, N, H, 0, .1, .5, .01, 2e-4, 1e-5, 40., 1, None)
    assert call(p=None) == 1 and call(n=3) == 1 and call(M=0) == 1 and call(E=-1, steps=0) == 1 and call(steps=9) == 1 and call(steps=-1) == 1
    assert call(N=0) == 1 and call(N=7) == 1 and call(H=0) == 1 and call(H=129) == 1
    assert callable(ops.ppo_update)


def test_refusals_that_need_no_device():
    from stove_amd import ops
    from stove_amd.rl import main_rl
    from stove_amd.rl.agents import PPOAgent
    from stove_amd.rl.rl_model import Policy
    batch = U.golden_batch(0)
    policy = U.golden_start(0)
    k = U.kernel_inputs(policy, batch)
    t = {key: torch.from_numpy(a) for key, a in k.items()}
    zeros = torch.zeros_like(t['image'])
    with pytest.raises(RuntimeError, match='GPU'):
        ops.ppo_update(t['image'], zeros, zeros.clone(), torch.zeros(1, dtype=torch.int32), t['obs'], t['actions'], t['returns'], t['values'],
                       t['logp'], t['adv'], t['perm'], 4, 64, False, .1, .5, .01, 2e-4, 1e-5, 40.)
    agent = PPOAgent(policy, .1, 2, 4, .5, .01, lr=2e-4, eps=1e-5, max_grad_norm=40, fused=True)
    before = {key: ten.clone() for key, ten in policy.state_dict().items()}
    col = lambda key: t[key].reshape(-1, 1)
    with pytest.raises(RuntimeError, match='GPU'):
        agent.update(t['obs'], col('actions').long(), col('returns'), col('values'), col('logp'), col('adv'))
    assert all(torch.equal(ten, before[key]) for key, ten in policy.state_dict().items())
    with pytest.raises(ValueError, match='fused=True'):
        PPOAgent(Policy((32, 32, 12), 9, hidden_size=512), .1, 2, 4, .5, .01, lr=2e-4, eps=1e-5, max_grad_norm=40, fused=True)
    # without the keyword (and with None / False) the agent is the torch one: same results under the same seed
    results = []
    for kw in ({}, {'fused': None}, {'fused': False}):
        p = U.golden_start(0)
        a = PPOAgent(p, .1, 2, 4, .5, .01, lr=2e-4, eps=1e-5, max_grad_norm=40, **kw)
        assert a.fused is False
        state = torch.get_rng_state()
        torch.manual_seed(0)
        losses = a.update(t['obs'], col('actions').long(), col('returns'), col('values'), col('logp'), col('adv'))
        torch.set_rng_state(state)
        results.append((losses, p.flat_params()))
    assert results[0][0] == results[1][0] == results[2][0] and torch.equal(results[0][1], results[1][1]) and torch.equal(results[0][1], results[2][1])
    assert not torch.equal(results[0][1], U.golden_start(0).flat_params())
    args = main_rl.parse_args(['--use-states', '--experiment_id', 'x', '--fused-update'])
    assert args.fused_update and not main_rl.parse_args(['--use-states', '--experiment_id', 'x']).fused_update
    with pytest.raises(ValueError, match='--fused-update'):
        main_rl.build(main_rl.parse_args(['--use-states', '--experiment_id', 'x', '--fused-update', '--device', 'cpu']))
