"""The control kernels (csrc/reward_head.hip, plan.hip, ppo_model.hip, ppo_model_cl.hip) against THEIR OWN results of an earlier build,
bit for bit: the reward head's forward, its table staging, the one-hot action embedding and the policy step between two imagined steps
are written out in several kernels (only the parameter layout, the dots and the embedding of one action are shared code); neither a
change to the shared code nor one to a copy may move a bit of what any of these kernels computes.

Yardstick: tests/golden/g29_control_bits.npz, recorded once by tools/make_control_bits_goldens.py on the build before the
kernels' shared pieces were moved into headers (see the tool's docstring for the commit).  Per case it holds the small CPU-seeded inputs, the SHA-256 of every
weight tensor and the SHA-256 of every output, so "equal" below is equality of digests, which is equality of bits, shape and dtype.
Every test first holds the inputs and weights it rebuilt to the fixture: a changed seed or initialiser shows as that, not as a kernel
change.

Shapes, the smallest that reach every caller:
  ops.reward_head forward   5 items (more than one block's four waves), 1 and 3 objects: reward and the saved H0, Q, A1, A2;
  ops.plan_expand           cl = 16, 32, 64; M = 2, A = 9, L = 2, D = 2, len_s = (1, 2); 1 and 3 objects, 6 at cl = 32; one tree with a
                            leaf index out of range (the NaN path): q, r_first, r_roll and the whole pool;
  ops.ppo_collect_model     B = 3, S = 3; cl = 32 at 1, 3, 5 and 6 objects (the one-object kernel, a wave per row, half-wave rows, the
                            unstaged 128-wide deep policy), cl = 16 and 64 at 1, 3 and 6; both activations at 3 objects; a trajectory
                            that starts from a NaN state (status, early exit, the tail); without and with `pred`: all ten outputs.

A digest says which tensor moved, not where or by how much: to see that, run the tool's run_* on both builds and compare.
"""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_tool():
    spec = importlib.util.spec_from_file_location('make_control_bits_goldens', os.path.join(ROOT, 'tools', 'make_control_bits_goldens.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load_tool()


@pytest.fixture(scope='module')
def fix():
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'g29_control_bits.npz')) as f:
        return {k: f[k] for k in f.files}


def _part(fix, prefix):
    return {k[len(prefix) + 1:]: v for k, v in fix.items() if k.startswith(prefix + '/')}


def _inputs_as_recorded(fix, key, inp):
    want = _part(fix, key + '/in')
    assert sorted(want) == sorted(inp), (key, sorted(inp), sorted(want))
    wrong = [k for k in want if not np.array_equal(G.digest(inp[k]), G.digest(want[k]))]
    assert not wrong, ('the inputs rebuilt are not the recorded ones', key, wrong)


def _same_bits(fix, key, got, weight_digests):
    want_w = _part(fix, key + '/w')
    assert sorted(want_w) == sorted(k[2:] for k in weight_digests), (key, sorted(weight_digests), sorted(want_w))
    wrong = [k for k in want_w if not np.array_equal(weight_digests['w/' + k], want_w[k])]
    assert not wrong, ('the weights rebuilt are not the recorded ones', key, wrong)
    want = _part(fix, key + '/out')
    assert want and sorted(want) == sorted(got), (key, sorted(got), sorted(want))
    wrong = [k for k in sorted(want) if not np.array_equal(G.digest(got[k]), want[k])]
    assert not wrong, (key, wrong)


@pytest.mark.parametrize('n', G.reward_head_cases())
def test_reward_head_forward_repeats_recorded_bits(fix, n):
    key = 'rh_n%d' % n
    inp = G.reward_head_inputs(n)
    _inputs_as_recorded(fix, key, inp)
    got, wd = G.run_reward_head(inp)
    assert sorted(got) == ['A1', 'A2', 'H0', 'Q', 'reward']
    _same_bits(fix, key, got, wd)


@pytest.mark.parametrize('cl,n,bad', G.plan_cases(), ids=lambda v: str(v))
def test_plan_expand_repeats_recorded_bits(fix, cl, n, bad):
    key = G.plan_key(cl, n, bad)
    inp = G.plan_inputs(cl, n, bad)
    _inputs_as_recorded(fix, key, inp)
    got, wd = G.run_plan(cl, n, inp)
    assert sorted(got) == ['pool', 'q', 'r_first', 'r_roll']
    _same_bits(fix, key, got, wd)


@pytest.mark.parametrize('cl,n,elu,nan', G.collect_cases(), ids=lambda v: str(v))
def test_imagined_collection_repeats_recorded_bits(fix, cl, n, elu, nan):
    key = G.collect_key(cl, n, elu, nan)
    inp = G.collect_inputs(cl, n, nan)
    _inputs_as_recorded(fix, key, inp)
    got, wd = G.run_collect_both(cl, n, elu, inp)
    assert sorted(got) == sorted([k for k in G.COLLECT_KEYS if k != 'pred'] + ['p/' + k for k in G.COLLECT_KEYS])
    _same_bits(fix, key, got, wd)
