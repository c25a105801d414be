"""The object SPN's table-gradient kernels (csrc/spn_obj.hip: objspn_tablegrad_under_k beside the recursion's backward, the wide
objspn_tablegrad_k everywhere else) against THEIR OWN results of an earlier build, bit for bit: changes to when a batch's operands are
fetched (software pipelining, lookahead into the next batch, a guard at a workgroup's last batch) must not move a bit of the three
gradients -- every accumulator keeps the order of its MFMAs over batches, h and e, and every operand its arithmetic.

Yardstick: tests/golden/g30_tablegrad_bits.npz, recorded once by tools/make_tablegrad_bits_goldens.py on the build before the under
kernel's batch loop was pipelined.  The inputs are large (16 384 frames are 64 MB), so it holds their seeds (frames in [0, 1], valid
z, a non-constant dll from torch's CPU generator; the tables are the analytic fill) and, for every result, the SHA-256 of its bytes,
so "equal" below is equality of digests, which is equality of bits (and of shape and dtype).  The call is the training pair
stove_scene_fwd_from + stove_scene_bwd_overlap with a parameter stream distinct from the main one.

Cases, the smallest at which a pipelined batch loop can go wrong -- the under kernel runs only with at most 4 objects and at least
16 384 glimpses, in 40 chunks, batch b in chunk b mod 40:
  1 object  x 16 384 frames   256 batches: 16 chunks get 7 batches and 24 get 6 (the lookahead's guard fires at different batches)
  3 objects x  5 462 frames   257 batches, the last with 2 live samples
  2 objects x  8 200 frames   the last batch with 16 live samples
  4 objects x  4 106 frames   the last batch with 40 live samples
  4 objects x  4 480 frames   280 batches: every chunk gets 7
and two for the wide kernel, whose tile staging (tg_stage_tile) the under kernel used to share: 3 objects x 43 frames (3 batches, fewer than its chunk count)
and 6 objects x 11 frames.  Checked per case: g_obj_coef, g_obj_wsum, g_obj_wroot; dz, g_bg_coef and g_bg_wroot as a check that
nothing else moved.

A digest says which tensor moved, not where or by how much: to see that, run the tool's run_case on both builds and compare.
"""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_tool():
    spec = importlib.util.spec_from_file_location('make_tablegrad_bits_goldens', os.path.join(ROOT, 'tools', 'make_tablegrad_bits_goldens.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load_tool()


@pytest.fixture(scope='module')
def fix():
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'g30_tablegrad_bits.npz')) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope='module')
def supairs():
    made = {}
    return lambda n_obj: made.setdefault(n_obj, G.make_supair(n_obj, DEV))


def test_cases_are_the_ones_the_batch_loop_can_go_wrong_at():
    """(no kernel runs: the arithmetic of the case list)"""
    shape = {}
    for n_obj, nf in G.UNDER_CASES:
        glimpses = n_obj * nf
        assert n_obj <= 4 and glimpses >= G.LATE
        batches = (glimpses + 63) // 64
        per_chunk = sorted({len(range(c, batches, G.CHUNKS)) for c in range(G.CHUNKS)})
        shape[(n_obj, nf)] = (batches, glimpses - 64 * (batches - 1), per_chunk)
    assert shape[(1, 16384)] == (256, 64, [6, 7])
    assert shape[(3, 5462)] == (257, 2, [6, 7])
    assert shape[(2, 8200)][1] == 16 and shape[(4, 4106)][1] == 40
    assert shape[(4, 4480)] == (280, 64, [7])
    for n_obj, nf in G.WIDE_CASES:
        assert n_obj * nf < G.LATE
    assert (3 * 43 + 63) // 64 == 3 and (6 * 11 + 63) // 64 == 2


@pytest.mark.parametrize('n_obj,nf', G.cases(), ids=lambda v: str(v))
def test_table_gradients_repeat_recorded_bits(fix, supairs, n_obj, nf):
    want = {k[len(G.key(n_obj, nf)) + 1:]: v for k, v in fix.items() if k.startswith(G.key(n_obj, nf) + '/')}
    assert sorted(want) == sorted(G.OUTPUTS + ('seed',))
    assert int(want['seed'][0]) == G.case_seed(n_obj, nf)
    got = G.run_case(supairs(n_obj), n_obj, nf, int(want['seed'][0]), DEV)
    assert sorted(got) == sorted(G.OUTPUTS)
    assert got['g_obj_coef'].numel() == 6 * 100 * 10 * 3 and got['dz'].shape == (nf * n_obj, 4)
    wrong = [k for k in G.OUTPUTS if not np.array_equal(G.digest(got[k]), want[k])]
    assert not wrong, (G.key(n_obj, nf), wrong)
