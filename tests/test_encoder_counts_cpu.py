"""What tests/test_gpu_encoder_counts.py and tests/test_gpu_model_counts.py rest on, checked without a GPU: the float64 restatement of
the LSTM cell (helpers.lstm_cell) against the oracle's recognition network and against torch.nn.LSTM at 1 .. 8 steps, the stated
ranges of the cell kernels' inputs, a scale for every max-norm comparison, the oracle's own decisions on the painted frames of the
model cases, and the coverage of the case lists."""
import numpy as np
import pytest
import torch

import stove_oracle as O
from helpers import (CELL_BWD_FORMS, CELL_FAST, CELL_FWD_FORMS, CELL_MORE, CELL_OUT_FORMS, CELL_PLANTS, CELL_REF_FORMS, CELL_SHAPES,
                     CHUNK_COUNTS, CHUNK_SIZES, COLSUM_COLS, COLSUM_ROWS, ENC_COUNTS, ENC_D, ENC_GEMMS, ENC_H, ENC_REGIMES, ENC_ROWS,
                     MODEL_COUNTS, MODEL_INIT_COUNTS, MODEL_SHAPES, cell_inputs, cell_reference, disc_radii, draw_tracks, encoder_cases,
                     encoder_dx_cases, encoder_inputs, encoder_product_paths, encoder_reference, lstm_cell_grads, lstm_chain, model_case_id,
                     model_cases, model_cfg, model_decisions, model_inputs, oracle_setup, paint_discs, rel_err, sum_inputs)

EPS64 = 2.0 ** -52


@pytest.mark.parametrize('K', ENC_COUNTS)
def test_cell_restatement_chained_is_the_oracles_recognition_network(K):
    """helpers.lstm_chain, K cell steps with no recurrent term and no previous cell at step 0, gives O.encoder_forward's hidden states
    bit for bit (the oracle adds a zero recurrent product and a zero cell there: x + 0 = x), in every weight regime"""
    x, _ = encoder_inputs(K, 37)
    for regime in ENC_REGIMES:
        c, _, params = oracle_setup(torch.float64, requires_grad=False, regime=regime, num_obj=K)
        _, hs = O.encoder_forward(c, params, x, hidden=True)
        b = params['sup.encoder.rnn.bias_ih_l0'] + params['sup.encoder.rnn.bias_hh_l0']
        got = lstm_chain(x.flatten(1) @ params['sup.encoder.rnn.weight_ih_l0'].t() + b, params['sup.encoder.rnn.weight_hh_l0'], K)
        assert got.shape == (37, K, ENC_H) and torch.equal(got, hs), regime
        assert torch.equal(hs, encoder_reference(K, 37, regime)['hs'])


@pytest.mark.parametrize('K', ENC_COUNTS)
def test_cell_restatement_chained_is_torch_lstm(K):
    """... and torch.nn.LSTM's in float64 on the frame repeated K times, to float64 rounding: 1e-12 of the largest hidden state"""
    x, _ = encoder_inputs(K, 37)
    for regime in ENC_REGIMES:
        c, _, params = oracle_setup(torch.float64, requires_grad=False, regime=regime, num_obj=K)
        rnn = torch.nn.LSTM(ENC_D, ENC_H).double()
        with torch.no_grad():
            for name, p in rnn.named_parameters():
                p.copy_(params['sup.encoder.rnn.' + name])
            want, _ = rnn(x.flatten(1).unsqueeze(0).expand(K, -1, -1))
        b = params['sup.encoder.rnn.bias_ih_l0'] + params['sup.encoder.rnn.bias_hh_l0']
        got = lstm_chain(x.flatten(1) @ params['sup.encoder.rnn.weight_ih_l0'].t() + b, params['sup.encoder.rnn.weight_hh_l0'], K)
        assert rel_err(got, want.transpose(0, 1)) < 1e-12, regime


def test_cell_backward_restatement_is_autograd_of_the_chain():
    """lstm_cell_grads step by step, the cell gradient handed from step to step, gives the gradient of the input projection that
    autograd finds through the whole chain (the sum of the steps' gate gradients: what dgx_sum is)"""
    K, n, H = 4, 5, 8
    g = torch.Generator().manual_seed(3)
    xp = torch.randn(n, 4 * H, generator=g, dtype=torch.float64)
    w_hh = torch.randn(4 * H, H, generator=g, dtype=torch.float64) * 0.3
    w = torch.randn(n, K, H, generator=g, dtype=torch.float64)
    xa = xp.clone().requires_grad_()
    hs = lstm_chain(xa, w_hh, K)
    (hs * w).sum().backward()
    cs, h, c = [], None, None
    for k in range(K):
        out = lstm_cell_grads(xp, None if h is None else h @ w_hh.t(), c, w[:, k])
        c, h = out['c'], out['h']
        cs.append(c)
    total, dh_rec, dc = torch.zeros_like(xp), torch.zeros(n, H, dtype=torch.float64), None
    for k in range(K - 1, -1, -1):
        out = lstm_cell_grads(xp, None if k == 0 else hs[:, k - 1].detach() @ w_hh.t(), cs[k - 1] if k else None, w[:, k] + dh_rec, dc)
        total, dc, dh_rec = total + out['dg'], out['dc_prev'], out['dg'] @ w_hh
    assert rel_err(total, xa.grad) < 64 * EPS64


@pytest.mark.parametrize('n,H', CELL_SHAPES)
def test_cell_inputs_meet_their_stated_ranges(n, H):
    """Pre-activations within [-3, 3] but for the planted entries, every planted value present in gx and in gh, previous cells in
    [-2, 2], float32 values throughout; and no reference output is all-zero or below 1e-3 in its largest entry"""
    x = cell_inputs(n, H)
    plants = torch.tensor(CELL_PLANTS, dtype=torch.float64).float().double()
    for k in ('gx', 'gh'):
        t = x[k].flatten()
        planted = (t.unsqueeze(1) == plants).any(1)
        assert float(t[~planted].abs().max()) <= 3.0 and int(planted.sum()) >= len(CELL_PLANTS)
        assert all(bool((t == v).any()) for v in plants), k
    assert float(x['c_prev'].abs().max()) <= 2.0 and float(x['dh'].abs().max()) <= 1.0 and float(x['dc_in'].abs().max()) <= 1.0
    assert x['dg_more'].shape == (CELL_MORE, n, 4 * H)
    for t in x.values():
        assert torch.equal(t, t.float().double())
    for gh, cp, dc in CELL_REF_FORMS:
        ref = cell_reference(n, H, gh, cp, dc)
        for k, v in ref.items():
            assert v.shape == ((n, 4 * H) if k == 'dg' else (n, H)) and float(v.abs().max()) > 1e-3, (k, gh, cp, dc)
        for m in (0, 1, 7):
            assert float((ref['dg'] + x['dg_more'][:m].sum(0)).abs().max()) > 1e-3


def test_reduction_inputs_have_a_scale():
    for rows in COLSUM_ROWS[1:]:
        for cols in COLSUM_COLS:
            assert float(sum_inputs(rows * 2000 + cols, rows, cols).sum(0).abs().max()) > 1e-3, (rows, cols)


def test_encoder_references_have_a_scale():
    """no gradient of the recognition network is all-zero -- the max norm of its comparison has a scale -- except W_hh at one step,
    which no product reads: exactly zero there"""
    for K in (1, 2, 8):
        for regime in ENC_REGIMES:
            ref = encoder_reference(K, 37, regime)
            assert float(ref['codes'].abs().max()) > 1e-3
            for name, gr in ref['grads'].items():
                if K == 1 and name == 'rnn.weight_hh_l0':
                    assert gr is None or not bool(gr.any())
                else:
                    assert float(gr.abs().max()) > 0, (K, regime, name)


def test_case_lists_cover_every_count_with_every_path():
    cases = encoder_cases()
    for K in ENC_COUNTS:
        mine = [c for c in cases if c[0] == K]
        assert {c[1] for c in mine} == set(ENC_ROWS) and {c[2] for c in mine} == set(ENC_REGIMES) == {'analytic', 'init', 'stress'}
        assert {c[3] for c in mine} == set(ENC_GEMMS) == {'bf16x3', 'fp32'} and {c[4] for c in mine} == {True, False}
        # both gradient paths at every count in every regime: into the arena's views inside the kernels, and through autograd
        for regime in ENC_REGIMES:
            direct = {encoder_product_paths(c[1], c[3], c[4])['direct'] for c in mine if c[2] == regime}
            assert direct == {True, False}
        assert sum(c[0] == K for c in encoder_dx_cases()) == 1
    assert len(cases) == 8 * 4 * 3 * 2 * 2
    assert {c[2] for c in encoder_dx_cases()} == set(ENC_REGIMES)
    assert CELL_SHAPES == [(1, 4), (3, 8), (37, 256), (257, 52), (2049, 256)] and set(CELL_FAST) == {0, 1}
    assert len(set(CELL_FWD_FORMS)) == 4 and len(set(CELL_REF_FORMS)) == 8 and len(set(CELL_BWD_FORMS)) == 40
    assert {o[0] for o in CELL_OUT_FORMS} == {True, False} and {o[1] for o in CELL_OUT_FORMS} == {None, 0, 1, 7}
    assert COLSUM_ROWS == (0, 1, 15, 16, 17, 511, 512, 513, 8193) and COLSUM_COLS == (1, 3, 8, 50, 64, 68, 1024)
    assert CHUNK_SIZES == (4, 1028) and CHUNK_COUNTS == (1, 2, 16, 17)
    mc = model_cases()
    assert len(set(mc)) == len(mc)
    for N in MODEL_COUNTS:
        mine = [c for c in mc if c[0] == N]
        assert {(c[1], c[2]) for c in mine} == set(MODEL_SHAPES) == {(3, 5), (1, 3)}
        assert {c[4] for c in mine if c[3] == 'analytic'} == {True, False}
        assert ('init' in {c[3] for c in mine}) == (N in MODEL_INIT_COUNTS)
        cfg = model_cfg(N)
        assert cfg.get('debug_match_objects', '3_only') == ('3_only' if N == 3 else 'greedy')
        assert (cfg.get('overlap_beta'), cfg.get('max_obj_scale')) == ((100.0, 0.22) if N > 3 else (None, None))
    assert set(MODEL_COUNTS) == set(range(1, 9)) and MODEL_INIT_COUNTS == (1, 4, 8)


@pytest.mark.parametrize('rows', ENC_ROWS)
def test_which_products_take_the_mfma_kernel(rows):
    """The row counts sit on both sides of ops.gemm_ok: the forward and dh products take the MFMA kernel at every row count unless
    encoder_gemm is 'fp32' (their sizes are 1024 and 256); the weight gradients run over the rows and take it at 256 and 300 only,
    and only there do the gradients go straight into the arena's views"""
    from stove_amd.ops import gemm_ok
    assert gemm_ok(ENC_D, ENC_H) and gemm_ok(rows) == (rows in (256, 300)) and gemm_ok(40)
    for arena in (True, False):
        p = encoder_product_paths(rows, 'bf16x3', arena, gemm_ok=gemm_ok)
        assert p == encoder_product_paths(rows, 'bf16x3', arena)
        assert p['forward'] == p['dh'] == 'mfma' and p['wgrad'] == ('mfma' if rows in (256, 300) else 'library')
        assert p['direct'] == (arena and rows in (256, 300))
        p = encoder_product_paths(rows, 'fp32', arena, gemm_ok=gemm_ok)
        assert set(p.values()) == {'library', False}
    assert not encoder_product_paths(40, 'bf16x3', True, needs_dx=True)['direct']            # a gradient of the input: autograd's path


def test_painter_gives_every_object_its_own_disc():
    """N discs of N radii: the painted area of object k alone is pi r_k^2 to a pixel's rim, dropping an object or swapping two radii
    changes the frame, and the channel sum stays in [0, 1]"""
    for N in MODEL_COUNTS:
        r = disc_radii(N)
        assert len(set(np.round(r, 6))) == N
        g = torch.Generator().manual_seed(N)
        tr = draw_tracks(g, 2, 4, N)
        assert tr.shape == (2, 4, N, 2) and float(np.abs(tr).max()) <= 0.8
        x = paint_discs(tr, r)
        assert x.shape == (2, 4, 3, 32, 32) and float(x.min()) >= 0 and float(x.max()) <= 1 and torch.equal(x, x.float().double())
        for k in range(N):
            one = paint_discs(tr[..., k:k + 1, :], r[k:k + 1])
            area = one.sum((-3, -2, -1))
            assert float((area - np.pi * r[k] ** 2).abs().max()) < 2.0 * np.pi * r[k] * 0.5 + 1.0
        if N > 1:
            assert not torch.equal(paint_discs(tr[..., :-1, :], r[:-1]), x)
            swapped = r.copy()
            swapped[[0, -1]] = swapped[[-1, 0]]
            assert not torch.equal(paint_discs(tr, swapped), x)
            assert not torch.equal(paint_discs(tr[..., ::-1, :].copy(), r), x)


MODEL_INPUT_KEYS = sorted({c[:4] for c in model_cases()})


@pytest.mark.parametrize('key', MODEL_INPUT_KEYS, ids=lambda k: 'N%d-B%dT%d-%s' % k)
def test_model_inputs_meet_the_input_condition(key):
    """On the chosen frames the oracle's float32 run returns the matching indices and the fix_supair hits of its float64 run, in
    every sequence of every case; every index is a permutation ('greedy' / '3_only')"""
    N, B, T, regime = key
    x, eps = model_inputs(N, B, T, regime)
    assert x.shape == (B, T, 3, 32, 32) and eps['latent'].shape == (B, N, 12, 1) and len(eps['steps']) == T - 2
    i64, h64 = model_decisions(N, regime, x, torch.float64)
    i32, h32 = model_decisions(N, regime, x, torch.float32)
    assert torch.equal(i64, i32) and torch.equal(h64, h32)
    assert bool((i64.sort(-1).values == torch.arange(N)).all())


def test_oracle_runs_at_one_object_and_at_one_sequence():
    """O.stove_forward keeps the object axis at N = 1 and the batch axis at B = 1 (its initial latents were squeezed)"""
    from helpers import oracle_stove
    for N, B, T in ((1, 3, 5), (1, 1, 3), (2, 1, 3)):
        x, eps = model_inputs(N, B, T, 'analytic')
        ref = oracle_stove(model_cfg(N), x, eps)
        assert ref['info']['z'].shape == (B, T - 2, N, 18) and bool(torch.isfinite(ref['elbo']))
        assert model_case_id((N, B, T, 'analytic', True)) == 'N%d-B%dT%d-analytic-fused' % (N, B, T)
