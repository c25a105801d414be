"""The small-graph recursion kernels (csrc/gnn_small.hip, gnn_small_bwd.hip) against THEIR OWN results of an earlier build, bit for
bit: changes to where those kernels load, wait and store (which wave issues a store, in which phase, behind which wait) must not move
a bit of what they compute or of the saved-activation and dY streams that gnn_dw_small_k turns into weight gradients.

Yardstick: tests/golden/g28_recursion_bits.npz, recorded once by tools/make_recursion_bits_goldens.py on the build before the node
rows' stores were moved behind the step's arithmetic.  It holds the CPU-seeded inputs, the weights (int16 numerators over 1024) and,
for every output, the SHA-256 of its bytes -- the weight gradients alone are 90 KB a case -- so "equal" below is equality of digests,
which is equality of bits (and of shape and dtype).

Shapes, the smallest at which a store hand-off can go wrong: B = 3 (more than one workgroup); 1 .. 6 objects (2 .. 6 are every
instantiation family of the small-graph kernels: wave 3 with and without a node row, two rows per wave at five and six; ONE object
runs the general dyn_loop_fwd_k / dyn_loop_bwd_k of gnn.hip, which the fixture pins all the same); Ts = 1, 2, 5 (a one-step loop,
both parities, an odd count); leaky-relu and elu; action-conditioned (23 inputs per node, `pred` and its gradient) at three and six
objects; the forward that saves its activations and the one that does not; the five-step cases again as the pieces [0, 2) + [2, 5)
through the kernels' ts0 / ts1 / carry arguments (stove_debug_set_piece), against the whole range's recorded bits; the mean rollout
and the sampling rollout (draws given, log_q recorded) over 3 steps at three and six objects.  Checked per case: z, zdyn, zdstd,
mean, stdv, pred; dz1, dzsup, dzsstd, dextra; the gradient images of all GNN weights and of all bias vectors.

A digest says which tensor moved, not where or by how much: to see that, run the tool's run_loop on both builds and compare.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_tool():
    spec = importlib.util.spec_from_file_location('make_recursion_bits_goldens', os.path.join(ROOT, 'tools', 'make_recursion_bits_goldens.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load_tool()
NL = (False, True)                  # leaky-relu, elu


@pytest.fixture(scope='module')
def fix():
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'g28_recursion_bits.npz')) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope='module')
def image(fix):
    return G.image_from(fix['w_num'], fix['v_num'], torch.device(DEV))


def _inputs(fix, prefix):
    return {k[len(prefix) + 1:]: v for k, v in fix.items() if k.startswith(prefix + '/')}


def _same_bits(got, fix, prefix, names=None):
    want = _inputs(fix, prefix)
    names = sorted(want) if names is None else names
    assert names and set(names) <= set(want) and set(names) <= set(got), (prefix, sorted(got), sorted(want))
    wrong = [k for k in names if not np.array_equal(G.digest(got[k]), want[k])]
    assert not wrong, (prefix, wrong)


@pytest.mark.parametrize('elu', NL, ids=['relu', 'elu'])
@pytest.mark.parametrize('n,ts,ac', G.loop_cases(), ids=lambda v: str(v))
def test_recursion_repeats_recorded_bits(fix, image, n, ts, ac, elu):
    inp = _inputs(fix, G.key(n, ts, ac))
    assert inp['zsup'].shape == (G.B, ts, n, 6) and ('extra' in inp) == bool(ac)
    got = G.run_loop(inp, image, elu)
    outputs = [k for k in G.OUTPUTS if k != 'pred' or ac]
    grads = [k for k in G.STATE_GRADS if k != 'dextra' or ac] + ['dW', 'dV']
    assert sorted(got) == sorted(outputs + grads)
    _same_bits(got, fix, G.key(n, ts, ac, elu))
    plain = G.run_loop(inp, image, elu, save=False)            # the forward that keeps nothing for a backward
    assert sorted(plain) == sorted(outputs)
    _same_bits(plain, fix, G.key(n, ts, ac, elu), outputs)


@pytest.mark.parametrize('elu', NL, ids=['relu', 'elu'])
@pytest.mark.parametrize('n,ac', G.rollout_cases(), ids=lambda v: str(v))
def test_mean_rollout_repeats_recorded_bits(fix, image, n, ac, elu):
    inp = _inputs(fix, 'roll_' + G.key(n, G.ROLLOUT_STEPS, ac))
    got = G.run_rollout(inp, image, elu)
    assert sorted(got) == sorted(['z_pred', 'zstd'] + (['pred'] if ac else []))
    _same_bits(got, fix, 'roll_' + G.key(n, G.ROLLOUT_STEPS, ac, elu))


@pytest.mark.parametrize('elu', NL, ids=['relu', 'elu'])
@pytest.mark.parametrize('n,ac', [(n, 0) for n in (2, 3, 4, 5, 6)] + [(n, 1) for n in G.AC_OBJECTS], ids=lambda v: str(v))
def test_recursion_in_pieces_repeats_the_whole_range(fix, image, n, ac, elu):
    """steps [0, 2) then [2, 5) forward, [2, 5) then [0, 2) backward: the state handed on in z, the gradient in the carry buffer"""
    ts = G.PIECES[-1]
    inp = _inputs(fix, G.key(n, ts, ac))
    assert inp['zsup'].shape == (G.B, ts, n, 6)
    got = G.run_loop_pieces(inp, image, elu)
    assert sorted(got) == sorted(_inputs(fix, G.key(n, ts, ac, elu)))
    _same_bits(got, fix, G.key(n, ts, ac, elu))


def test_piece_outside_the_steps_is_refused(fix, image):
    inp = _inputs(fix, G.key(3, 2, 0))
    with pytest.raises(RuntimeError, match='stove_dynloop_fwd'):
        G.run_loop_pieces(inp, image, False, bounds=(0, 5))           # the tensors hold two steps


@pytest.mark.parametrize('elu', NL, ids=['relu', 'elu'])
@pytest.mark.parametrize('n,ac', G.rollout_cases(), ids=lambda v: str(v))
def test_sampling_rollout_repeats_recorded_bits(fix, image, n, ac, elu):
    inp = _inputs(fix, 'sroll_' + G.key(n, G.ROLLOUT_STEPS, ac))
    assert inp['eps'].shape == (G.B, G.ROLLOUT_STEPS, n, 16)
    got = G.run_rollout(inp, image, elu, sample=True)
    assert sorted(got) == sorted(['z_pred', 'zstd', 'log_q'] + (['pred'] if ac else []))
    _same_bits(got, fix, 'sroll_' + G.key(n, G.ROLLOUT_STEPS, ac, elu))
