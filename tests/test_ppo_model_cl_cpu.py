"""CPU-side checks (-m "not gpu") of the model-based PPO arm on models of state-code length 16 and 64: the host specification on 10-
and 34-wide states, the argument checks of ops.ppo_collect_model that need no GPU, the C ABI addition (header, library, binding
table, ABI_VERSION still 7), its argument checks under the sanitizers (tests/abi/ppo_model_cl_validate_driver.cpp) and the switch
`fused_widths` of the runner and of main_rl.  (All fail before the feature: the entry point, the widened shapes and the attribute do
not exist.)"""
import ctypes
import types

import numpy as np
import pytest
import torch

import control_harness
import ppo_cases as P

HW = 10.0
WIDTHS = {16: 10, 64: 34}          # cl -> the width of a state row, cl/2 + 2


def _states(K, N, width, seed):
    rs = np.random.RandomState(seed)
    z = rs.uniform(-1.2, 1.2, (K, N, width)).astype(np.float32)
    z[:, :, :2] = 0.1
    return z


# ------------------------------------------------------------------------------------------------ 1. the host specification
@pytest.mark.parametrize('width', sorted(WIDTHS.values()))
@pytest.mark.parametrize('N,H,deep', [(1, 32, False), (3, 64, False), (6, 128, True)])
def test_decide_model_reads_columns_2_to_5_at_every_width(width, N, H, deep):
    """decide_model / observe_model on 10- and 34-wide states equal the same call on an 18-wide array that carries the same columns
    2 .. 5 (and other values everywhere else), bit for bit"""
    from stove_amd.rl.collect import PolicyForest, uniforms
    K = 16
    forest = PolicyForest.from_policy(P.policy(N, H, deep))
    z = _states(K, N, width, 500 + width + N)
    twin = _states(K, N, 18, 900 + N)
    twin[:, :, 2:6] = z[:, :, 2:6]
    u = uniforms(K, 1, 600 + N)[:, 0]
    got, want = forest.decide_model(z, HW, u), forest.decide_model(twin, HW, u)
    assert len(got) == len(want) == 5
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    assert len(set(got[2].tolist())) > 1 or K == 1               # (the draw matters)
    a, b = PolicyForest.observe_model(z, HW), PolicyForest.observe_model(twin, HW)
    assert a.dtype == np.float32 and a.shape == (K, 4 * N) and a.tobytes() == b.tobytes() == got[0].tobytes()


def test_decide_model_still_refuses_other_shapes():
    from stove_amd.rl.collect import PolicyForest
    forest = PolicyForest.from_policy(P.policy(3, 64, False))
    u = np.zeros(4, np.float32)
    for shape in ((4, 3, 17), (4, 3, 26), (4, 3, 66), (4, 3, 9), (4, 2, 10), (4, 2, 34), (4, 30), (4, 3, 10, 1)):
        with pytest.raises(ValueError, match='the policy reads'):
            forest.decide_model(np.zeros(shape, np.float32), HW, u)
    for width in (10, 18, 34):
        with pytest.raises(ValueError, match='float32 vector of 4 uniforms'):
            forest.decide_model(np.zeros((4, 3, width), np.float32), HW, np.zeros(4))


# ------------------------------------------------------------------------------------------------ 2. ops: what the host can check
@pytest.mark.parametrize('cl', sorted(WIDTHS))
def test_ops_ppo_collect_model_checks_its_arguments_on_the_host(cl):
    from stove_amd import ops
    z0 = torch.zeros(3, 3, WIDTHS[cl])
    image = torch.zeros(8554)
    rest = lambda: (None, image, torch.zeros(12, 9), torch.zeros(12), torch.zeros(10), torch.zeros(10), torch.zeros(3, 5), 64, False, 2, False,
                    (0.3, 0.04, 0.04), HW)
    for width in (9, 17, 26, 66):
        with pytest.raises(ValueError, match=r'z0 must be a \(B, N, 18\) tensor'):
            ops.ppo_collect_model(torch.zeros(3, 3, width), *rest())
    with pytest.raises(ValueError, match=r'z0 must be a \(B, N, 18\) tensor'):
        ops.ppo_collect_model(z0.numpy(), *rest())
    with pytest.raises(ValueError, match=r'z0 must be a \(B, N, 18\) tensor'):
        ops.ppo_collect_model(z0[0], *rest())
    with pytest.raises(RuntimeError, match='forward only'):
        ops.ppo_collect_model(z0.clone().requires_grad_(True), *rest())
    # a state of a served width passes the shape check and is then asked for on the GPU (the sizes are checked there:
    # tests/test_gpu_ppo_model_cl.py)
    with pytest.raises(RuntimeError, match='GPU'):
        ops.ppo_collect_model(z0, *rest())


# ------------------------------------------------------------------------------------------------ 3. header, library, binding table
def test_the_entry_point_in_header_library_and_binding():
    from stove_amd import _lib, build
    build.build_library()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    name = 'stove_ppo_collect_model_cl'
    ret, params = control_harness.header_decl(name)
    assert ret == 'int' and len(params) == 33 and params[0] == 'const float* z0' and params[-1] == 'void* stream'
    # the `_cl` convention: the cl = 32 call's parameters with `int cl` between the pointers and the first size
    base = control_harness.header_decl('stove_ppo_collect_model')[1]
    lead = next(k for k, p in enumerate(base) if '*' not in p)
    assert lead == 18 and params == base[:lead] + ['int cl'] + base[lead:]
    assert hasattr(raw, name)

    class Recorder:
        def __init__(self):
            self.bound = {}

        def __getattr__(self, name):
            return self.bound.setdefault(name, types.SimpleNamespace())
    rec = Recorder()
    _lib._declare(rec)
    args = rec.bound[name].argtypes
    assert len(args) == 33 and args[18:27] == [ctypes.c_int] * 9 and args[27:32] == [ctypes.c_float] * 5
    assert len(rec.bound['stove_ppo_collect_model'].argtypes) == 32
    assert _lib.ABI_VERSION == 7 and _lib.load().stove_abi_version() == 7
    # the two empty-call forms need no device: B == 0 launches nothing; a width without kernels is refused before anything else
    lib = _lib.load()
    tail = (8, 3, 64, 0, 3, 2, 0, 0.3, 0.04, 0.04, 10.0, 0.95, None)
    for cl in WIDTHS:
        assert lib.stove_ppo_collect_model_cl(*([None] * 18), cl, 0, *tail) == 0
    for cl in (32, 48, 0):
        assert lib.stove_ppo_collect_model_cl(*([None] * 18), cl, 0, *tail) == 1          # hipErrorInvalidValue


def test_argument_checks_under_the_sanitizers(tmp_path_factory):
    """csrc/validate.h: ppo_collect_model_cl compiled host-only with -fsanitize=address,undefined and driven by a stand-alone program:
    every documented rejection, the two empty-call forms, nothing dereferenced"""
    control_harness.run_modes(control_harness.build_driver(tmp_path_factory, 'ppo_model_cl_validate_driver'), ['validate'])


# ------------------------------------------------------------------------------------------------ 4. the switch
def _stub(cl, num_obj=3, cuda=True):
    """what fused_serves_model looks at: the configuration and the first parameter's device and dtype"""
    c = types.SimpleNamespace(cl=cl, num_obj=num_obj, debug_core_appearance=True, debug_appearance_dim=3, action_conditioned=True, action_space=9)
    p = types.SimpleNamespace(is_cuda=cuda, dtype=torch.float32)
    return types.SimpleNamespace(c=c, parameters=lambda: iter([p]))


def test_the_runners_width_switch_on_a_stub_model():
    """fused_widths: (32,) by default -- today's answers --, a tuple to assign; fused_serves_model hands it to _fused_unserved (a runner
    on the host serves nothing: its device is asked first, so the device is faked here)"""
    from stove_amd.mcts import mcts_stove
    from stove_amd.rl import main_rl
    runner, _ = main_rl.build(main_rl.parse_args(['--use-pretrained-model', '--experiment_id', 'x', '--checkpoint', 'a', '--data', 'b',
                                                  '--device', 'cpu']))
    assert runner.fused_widths == mcts_stove.FUSED_WIDTHS == (32,)
    assert not any(runner.fused_serves_model(_stub(cl)) for cl in (16, 32, 64))            # a host runner
    runner.device = torch.device('cuda:0')                                                   # (nothing is launched)
    assert [runner.fused_serves_model(_stub(cl)) for cl in (16, 32, 64)] == [False, True, False]
    runner.fused_widths = (16, 32, 64)
    assert [runner.fused_serves_model(_stub(cl)) for cl in (16, 32, 64, 48)] == [True, True, True, False]
    assert not runner.fused_serves_model(_stub(16, num_obj=7)) and not runner.fused_serves_model(_stub(64, cuda=False))
    runner.fused_widths = (64,)
    assert [runner.fused_serves_model(_stub(cl)) for cl in (16, 32, 64)] == [False, False, True]
    # fused=True on a width that is not offered: a ValueError that names the width, before anything touches a device
    runner.fused_widths = (32,)
    for cl in (16, 64):
        with pytest.raises(ValueError, match='cl = %d' % cl):
            runner.collect_model(_stub(cl), torch.zeros(2, 3, cl // 2 + 2), None, fused=True, u=np.zeros((2, runner.num_steps), np.float32))


def test_main_rl_takes_fused_widths():
    from stove_amd.rl import main_rl
    base = ['--use-pretrained-model', '--experiment_id', 'x', '--checkpoint', 'run_dir', '--data', 'seq.pkl', '--device', 'cpu']
    args = main_rl.parse_args(base)
    assert args.fused_widths is None and main_rl.build(args)[0].fused_widths == (32,)
    args = main_rl.parse_args(base + ['--fused-widths', '16,32,64'])
    assert args.fused_widths == (16, 32, 64)
    runner, policy = main_rl.build(args)
    assert runner.fused_widths == (16, 32, 64) and policy.kernel_shape() == (3, 64, False)
    assert main_rl.parse_args(base + ['--fused-widths', '64']).fused_widths == (64,)
    import json
    json.dumps(vars(args))                                                               # (save_args writes them)
