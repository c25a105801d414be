"""CPU side of the state-supervised baseline: tests/sup_ref.py and the data set's supervised rescaling against what the reference's
own code gives (tests/golden/g31_supervised_f64.npz, tools/make_sup_goldens.py), the entry point's configuration and refusals, the new
C entry points in header, library and binding table, their argument checks under the sanitizers (tests/abi/sup_validate_driver.cpp),
and the conditioning of the inputs that tests/test_gpu_sup.py runs (tests/sup_cases.py)."""
import types

import numpy as np
import pytest
import torch

import control_harness
import sup_cases as C
import sup_ref as S
from gpu_helpers import err, err_l2, err_small
from helpers import load_golden, rel_err

ENTRY_POINTS = {'stove_sup_rollout_fwd': ('int', 12), 'stove_sup_rollout_bwd_ws_bytes': ('size_t', 3), 'stove_sup_rollout_bwd': ('int', 14),
                'stove_sup_loss': ('int', 11)}
GOLDEN_CASES = [(shape, fill, nl) for shape in ((3, 4, 3, 4), (2, 2, 1, 1)) for fill in ('init', 'half') for nl in C.NL]


@pytest.fixture(scope='module')
def g31():
    return load_golden('g31_supervised_f64')


# ------------------------------------------------------------------------------------------------ the restatement and the data set
@pytest.mark.parametrize('shape,fill,nl', GOLDEN_CASES, ids=lambda v: '-'.join(map(str, v)) if isinstance(v, tuple) else v)
def test_sup_ref_against_the_reference(g31, shape, fill, nl):
    """sup_rollout_ref + sup_loss_ref on the fixture's inputs: pred, the three losses and every parameter gradient of the total at
    1e-10; the reference differentiates exactly the 28 tensors of the encoder and core 0"""
    N, B, V, R = shape
    key = 'n%dB%dV%dR%d_%s_%s/' % (N, B, V, R, fill, nl)
    x, lat, fut = (torch.from_numpy(g31[key + k]) for k in ('x', 'latent0', 'future'))
    assert x.shape == (B, V, N, 4) and lat.shape == (B, N, 12) and fut.shape == (B, R, N, 4)
    params = S.sup_params(16, fill)
    pred = S.sup_rollout_ref(S.sup_config(16, nl, num_obj=N), params, x, lat, R)
    total, pred_loss, delta_loss = S.sup_loss_ref(pred, fut, C.DISCOUNT)
    assert rel_err(pred.detach(), g31[key + 'pred']) < 1e-10
    want = g31[key + 'losses']
    assert want[2] == 0.0                                    # the reference's reconstruction term: mse(x, x)
    assert rel_err(total.item(), want[0]) < 1e-10 and rel_err(pred_loss.item(), want[1]) < 1e-10
    assert rel_err((pred_loss + delta_loss).item(), want[0]) < 1e-10
    assert (delta_loss.item() == 0.0) == (R == 1)
    total.backward()
    grads = {k[len(key) + 5:]: v for k, v in g31.items() if k.startswith(key + 'grad/')}
    assert set(grads) == set(params) and len(grads) == 28
    for k, g in grads.items():
        if np.abs(g).max() == 0.0:                           # (cannot happen at N >= 2)
            assert float(params[k].grad.abs().max()) == 0.0
        else:
            assert rel_err(params[k].grad, g) < 1e-10, k


def _ds_config(**kw):
    from stove_amd.supairvised.config import SupStoveConfig
    c = SupStoveConfig()
    c.num_visible, c.num_rollout, c.num_episodes = 3, 4, 1000
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_dataset_rescaling_against_the_reference(g31):
    from stove_amd.video_prediction.load_data import StoveDataset
    data = {'X': g31['ds_X'].copy(), 'y': g31['ds_y'].copy()}
    ds = StoveDataset(_ds_config(), data=data)
    assert ds.total_data.shape == (2, 20, 3, 4) and ds.total_img.shape == (2, 20, 1, 8, 8)
    assert np.abs(ds.total_data - g31['ds_total_data']).max() < 1e-12
    assert np.abs(ds.total_img - g31['ds_total_img']).max() < 1e-12
    sample = ds[3]
    keys = [k[len('ds_sample/'):] for k in g31 if k.startswith('ds_sample/')]
    assert sorted(sample) == sorted(keys)
    for k in keys:
        assert np.abs(np.asarray(sample[k]) - g31['ds_sample/' + k]).max() < 1e-12, k
    assert np.array_equal(data['y'], g31['ds_y'])              # the caller's arrays are left alone


def test_dataset_without_the_flag_is_unchanged(g31):
    """supairvised = False gives what a config without the attribute gives: the [-1, 1] frame and the colour frames"""
    from stove_amd.video_prediction.load_data import StoveDataset
    data = {'X': g31['ds_X'], 'y': g31['ds_y']}
    off = StoveDataset(_ds_config(supairvised=False), data=data)
    c = types.SimpleNamespace(**{k: getattr(_ds_config(), k) for k in ('num_visible', 'num_rollout', 'num_episodes', 'frame_step', 'debug_add_noise')})
    absent = StoveDataset(c, data=data)
    assert np.array_equal(off.total_data, absent.total_data) and np.array_equal(off.total_img, absent.total_img)
    want = g31['ds_y'] * (2 / 10)
    want[..., :2] -= 1
    assert np.array_equal(off.total_data, want) and off.total_img.shape == (2, 20, 3, 8, 8)


# ------------------------------------------------------------------------------------------------ entry point, refusals
def test_main_builds_the_supervised_configuration():
    from stove_amd import main as M
    from stove_amd.supairvised.config import SupStoveConfig
    dtype, threads = torch.get_default_dtype(), torch.get_num_threads()
    try:                                                     # (build_config sets the process's default dtype and thread count)
        c = M.build_config({'supairvised': 'True', 'nolog': 'True', 'random_seed': '5'})
        assert isinstance(c, SupStoveConfig) and c.cl == 16 and c.num_visible == 6 and c.supairvised is True
        assert c.discount_factor == 0.98 and c.debug_rollout and c.debug_rollout_training and c.debug_anneal_lr == 20000
        plain = M.build_config({'nolog': 'True', 'random_seed': '5'})
        assert not isinstance(plain, SupStoveConfig) and plain.cl == 32 and plain.num_visible == 8
        with pytest.raises(NotImplementedError, match='out of scope'):
            M.build_config({'supairvised': 'True', 'load_encoder': 'some/ckpt', 'nolog': 'True', 'random_seed': '5'})
    finally:
        torch.set_default_dtype(dtype)
        torch.set_num_threads(threads)


def _model_config(**kw):
    c = _ds_config(num_obj=3, device=torch.device('cpu'), dtype=torch.float32, action_conditioned=False, action_space=None)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_model_refusals():
    from stove_amd.supairvised.dynamics import SupervisedDynamics
    from stove_amd.supairvised.supstove import SupStove
    with pytest.raises(NotImplementedError, match='action'):
        SupervisedDynamics(_model_config(action_conditioned=True, action_space=9))
    with pytest.raises(NotImplementedError, match='debug_core_appearance'):
        SupervisedDynamics(_model_config(debug_core_appearance=True))
    with pytest.raises(NotImplementedError, match='cl in'):
        SupervisedDynamics(_model_config(cl=32))
    with pytest.raises(NotImplementedError, match='out of scope'):
        SupStove(_model_config(load_encoder='some/ckpt'))
    st = SupStove(_model_config())
    assert not hasattr(st, 'sup') and st.dyn.enc_input_size == 16 and tuple(st.dyn.state_enc.weight.shape) == (16, 16)
    assert len(list(st.dyn.named_parameters())) == 2 + 3 * 26
    x = torch.zeros(2, 3, 3, 4)
    with pytest.raises(ValueError, match='debug_rollout=True only'):
        st.dyn(x, num_rollout=2, debug_rollout=False)
    with pytest.raises(NotImplementedError, match='action'):
        st.dyn(x, num_rollout=2, actions=torch.zeros(2, 5, 9))
    wide = SupervisedDynamics(_model_config(cl=64))           # (no transition_lik_std of 32 entries is asked for)
    assert wide.enc_input_size == 64


def test_model_package_re_exports():
    import model.supairvised.config as mc
    import model.supairvised.dynamics as md
    import model.supairvised.supstove as ms
    import model.supairvised.train as mt
    from stove_amd.supairvised import config, dynamics, supstove, train
    assert mc.SupStoveConfig is config.SupStoveConfig and md.SupervisedDynamics is dynamics.SupervisedDynamics
    assert ms.SupStove is supstove.SupStove and mt.SupTrainer is train.SupTrainer


def test_trainer_loss_in_plain_torch_follows_the_restatement():
    """compute_loss off the GPU (float64): the restatement's total and pred loss under every switch; `its` inverts the data set's scaling"""
    from stove_amd.supairvised.train import SupTrainer
    d = C.inputs((16, 3, 11, 3, 4, 'init', 'relu'))
    pred = d['future'] + 0.1 * d['w']
    for v_err in (False, True):
        for v_diff in (False, True):
            stub = types.SimpleNamespace(c=_model_config(debug_disable_v_error=v_err, debug_disable_v_diff_error=v_diff))
            total, pred_loss, recon = SupTrainer.compute_loss(stub, d['x'], d['future'], d['x'], pred)
            want = S.sup_loss_ref(pred, d['future'], 0.98, 2 if v_err else 4, not v_diff)
            assert recon.item() == 0.0 and rel_err(total.item(), want[0].item()) < 1e-13 and rel_err(pred_loss.item(), want[1].item()) < 1e-13
    y = torch.tensor([[3.0, 8.0, -1.0, 0.5]])
    scaled = torch.cat([y[:, :2] / 5, y[:, 2:] * 2], -1)
    assert torch.allclose(SupTrainer.its(scaled), torch.cat([y[:, :2] / 5 - 1, y[:, 2:] / 5], -1))


# ------------------------------------------------------------------------------------------------ C ABI
def test_entry_points_are_declared_exported_and_bound():
    import ctypes
    from stove_amd import _lib, build
    build.build_library()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    rec = types.SimpleNamespace()

    class Recorder:
        def __getattr__(self, name):
            return rec.__dict__.setdefault(name, types.SimpleNamespace())
    _lib._declare(Recorder())
    for name, (ret, count) in ENTRY_POINTS.items():
        decl = control_harness.header_decl(name)
        assert decl[0] == ret and len(decl[1]) == count, (name, decl)
        assert hasattr(raw, name) and len(getattr(rec, name).argtypes) == count, name
    names = [p.split()[-1].lstrip('*') for p in control_harness.header_decl('stove_sup_rollout_bwd')[1]]
    assert names == ['x', 'params', 'codes', 'd_pred', 'd_latent0', 'g_params', 'ws', 'cl', 'B', 'V', 'R', 'N', 'elu', 'stream']
    assert control_harness.header_decl('stove_sup_loss')[1][-2] == 'double discount'
    assert _lib.ABI_VERSION == 7 == _lib.load().stove_abi_version()


def test_workspace_query_rejects_what_the_call_rejects():
    from stove_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    for cl in (16, 64):
        for B, N in ((1, 1), (11, 3), (11, 5), (256, 6), (600, 2)):
            assert lib.stove_sup_rollout_bwd_ws_bytes(cl, B, N) == lib.stove_gnn_bwd_ws_bytes_cl(cl, B, N) > 0, (cl, B, N)
        for B, N in ((0, 3), (-1, 3), (4, 0), (4, 7)):
            assert lib.stove_sup_rollout_bwd_ws_bytes(cl, B, N) == 0, (cl, B, N)
    for cl in (32, 48, 0):
        assert lib.stove_sup_rollout_bwd_ws_bytes(cl, 11, 3) == 0


def test_argument_checks_under_the_sanitizers(tmp_path_factory):
    exe = control_harness.build_driver(tmp_path_factory, 'sup_validate_driver')
    control_harness.run_modes(exe, ['validate'])


# ------------------------------------------------------------------------------------------------ the GPU cases' inputs
def test_the_case_list_covers_what_it_has_to():
    cases = C.cases()
    assert len(cases) == 14 and len({C.case_id(c) for c in cases}) == 14
    assert {c[0] for c in cases} == {16, 64} and {c[1] for c in cases} == {1, 2, 3, 5, 6}
    assert (16, 3, 11, 6, 8) in {c[:5] for c in cases}                                   # the reference's V and R
    for c in cases:
        assert (c[5] == 'analytic') == C.one_step(c)                                     # plain 'analytic' in one-step cases only
    for fill in ('init', 'half'):
        assert {c[6] for c in cases if c[5] == fill} == set(C.NL)
    assert {c[6] for c in cases if c[0] == 64} == set(C.NL) == {c[6] for c in cases if c[0] == 16}


@pytest.mark.parametrize('case', C.cases(), ids=C.case_id)
def test_gpu_case_inputs_are_well_conditioned(case):
    """the float32 run of sup_ref against its float64 run: regime_bar lifts no bar of the GPU test beyond CAP x its base"""
    d = C.inputs(case)
    hi, lo = C.ref_case(case, torch.float64, d), C.ref_case(case, torch.float32, d)
    gap = err(lo['pred'], hi['pred'])
    base = C.PRED_BAR_STEP if C.one_step(case) else C.PRED_BAR_ROLLOUT
    gaps = [max(f(lo[k][n], hi[k][n]) for k in ('g_total', 'g_w') for n in hi[k]) for f in (err, err_l2, err_small)]
    print('%s: pred gap %.3g, gradient gaps %s' % (C.case_id(case), gap, ' '.join('%.3g' % g for g in gaps)))
    assert C.MULT * gap <= C.CAP * base, gap
    for g, b in zip(gaps, C.GRAD_BARS):
        assert C.MULT * g <= C.CAP * b, (g, b)
    assert float(hi['pred'].abs().max()) < 50.0               # the rollout stays bounded
