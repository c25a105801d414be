"""The recognition network at EVERY number of LSTM steps the model can ask for (the number of objects, 1 .. 8), where the other tests
run three (and six in the chunk-equality test), and its cell and reduction kernels on their own.

1. stove_lstm_cell_fwd / _bwd through the C ABI against helpers.lstm_cell_grads, the float64 restatement of the oracle's cell
   (pinned to O.encoder_forward and torch.nn.LSTM by tests/test_encoder_counts_cpu.py): five (n, H) shapes -- one thread, a partial
   workgroup, ragged tails over several workgroups, an H that is no multiple of 64 --, every null form of gh, c_prev, dc_in, dg and
   dgx_sum, n_more = 0 / 1 / 7, fast = 0 and 1 on the same inputs at the same bars.  Every output starts as nan and must come back
   written; two calls agree bit for bit.
2. RnnStates at K = 1 .. 8 steps x rows 1 / 37 / 256 / 300 x the three weight regimes x encoder_gemm 'bf16x3' / 'fp32' x the
   parameter arena on / off, against O.encoder_forward in float64: codes and all eight parameter gradients; ops.encoder_lstm with the
   gradient of its input at every K; at one step the gradient of W_hh is exactly zero and the arena's slice keeps what it held.
3. the reductions that finish this backward (ops.colsum, stove_colsum2, stove_sum_chunks) against float64 sums at the level
   boundaries of colsum_level and both part kernels.

Bars: the project's for element-wise kernels (1e-6 values, 1e-5 gradients) and test_encoder_lstm_against_oracle's for the network
(codes 1.2e-5, gradients 4e-5 / 3e-5 / 1.2e-3), or 6 x what the reference's own float32 run differs from its float64 run by on the
same inputs where that is larger (gpu_helpers.regime_bar); the gap is measured on the CPU and printed next to the achieved error."""
import pytest
import torch

from gpu_helpers import check_ratio, err, err_l2, err_small, fill_analytic, regime_bar
from helpers import (CELL_BWD_FORMS, CELL_FAST, CELL_FWD_FORMS, CELL_MORE, CELL_SHAPES, CHUNK_COUNTS, CHUNK_SIZES, COLSUM_COLS, COLSUM_ROWS,
                     ENC_COUNTS, ENC_GEMMS, ENC_H, ENC_REGIMES, ENC_ROWS, cell_inputs, cell_reference, encoder_dx_cases, encoder_inputs,
                     encoder_product_paths, encoder_reference, lstm_chain, oracle_setup, sum_inputs)
from test_gpu_dynamics import make_cfg

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN = float('nan')


def _dev(t):
    return None if t is None else t.float().to(DEV).contiguous()


def _held(key, got, want, low, bar, case=''):
    """check(got against the float64 reference `want`) at regime_bar(bar, the reference's own float32 gap); both are printed"""
    e, gap = err(got, want), err(low, want)
    print(f'{key} {case}: {e:.3g} (reference f32 gap {gap:.3g}, bar {regime_bar(bar, gap):.3g})')
    check_ratio(key, e, regime_bar(bar, gap))


def _held_grad(key, got, want, low, case=''):
    """a gradient tensor on three scales (gpu_helpers.check_grad's), each at its bar or 6 x the reference's float32 gap on that scale"""
    for sfx, fn, bar in (('', err, 4e-5), ('.l2', err_l2, 3e-5), ('.small', err_small, 1.2e-3)):
        e, gap = fn(got, want), fn(low, want)
        if gap > bar / 6:
            print(f'{key}{sfx} {case}: {e:.3g} (reference f32 gap {gap:.3g}, bar {regime_bar(bar, gap):.3g})')
        check_ratio(key + sfx, e, regime_bar(bar, gap))


def _lib():
    from stove_amd import _lib
    return _lib.load(), _lib.ptr, _lib.stream


# ------------------------------------------------------------------------------------------------ 1. the cell kernels through the C ABI
def _cell_fwd(x, n, H, cp, gh, fast):
    lib, p, stream = _lib()
    c, h = torch.full((n, H), NAN, device=DEV), torch.full((n, H), NAN, device=DEV)
    rc = lib.stove_lstm_cell_fwd(p(x['gx']), p(x['gh']) if gh else None, p(x['c_prev']) if cp else None, p(c), p(h), n, H, fast, stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert not torch.isnan(c).any() and not torch.isnan(h).any(), 'elements the kernel did not write'
    return c, h


@pytest.mark.parametrize('fast', CELL_FAST)
@pytest.mark.parametrize('n,H', CELL_SHAPES)
def test_cell_forward_against_the_restatement(n, H, fast):
    x = {k: _dev(v) for k, v in cell_inputs(n, H).items()}
    for cp, gh in CELL_FWD_FORMS:
        ref, low = cell_reference(n, H, gh, cp, False), cell_reference(n, H, gh, cp, False, torch.float32)
        c, h = _cell_fwd(x, n, H, cp, gh, fast)
        key, case = f'cell.fwd.n{n}H{H}.fast{fast}', f'cp{int(cp)}gh{int(gh)}'
        _held(key + '.c', c, ref['c'], low['c'], 1e-6, case)
        _held(key + '.h', h, ref['h'], low['h'], 1e-6, case)
        c2, h2 = _cell_fwd(x, n, H, cp, gh, fast)
        assert torch.equal(c, c2) and torch.equal(h, h2)


def _cell_bwd(x, c, n, H, form, fast):
    """-> dict of the outputs the form asks for (dg, dgx_sum) and dc_out; every one starts as nan"""
    lib, p, stream = _lib()
    gh, cp, dc, store_dg, n_more = form
    out = {'dc_prev': torch.full((n, H), NAN, device=DEV)}
    if store_dg:
        out['dg'] = torch.full((n, 4 * H), NAN, device=DEV)
    if n_more is not None:
        out['dgx_sum'] = torch.full((n, 4 * H), NAN, device=DEV)
    rc = lib.stove_lstm_cell_bwd(p(x['gx']), p(x['gh']) if gh else None, p(x['c_prev']) if cp else None, p(c), p(x['dh']),
                                 p(x['dc_in']) if dc else None, p(out['dg']) if store_dg else None, p(out['dc_prev']),
                                 p(out['dgx_sum']) if n_more is not None else None, p(x['dg_more']) if n_more else None,
                                 n_more or 0, n, H, fast, stream())
    assert rc == 0
    torch.cuda.synchronize()
    for k, v in out.items():
        assert not torch.isnan(v).any(), k + ' holds elements the kernel did not write'
    return out


@pytest.mark.parametrize('fast', CELL_FAST)
@pytest.mark.parametrize('n,H', CELL_SHAPES)
def test_cell_backward_against_the_restatement(n, H, fast):
    """The backward reads the cell state the FORWARD of the same form stored (the float64 reference's, rounded to float32: the
    backward kernel is held on its own, not behind the forward kernel's rounding)."""
    x64 = cell_inputs(n, H)
    x = {k: _dev(v) for k, v in x64.items()}
    for form in CELL_BWD_FORMS:
        gh, cp, dc, store_dg, n_more = form
        ref, low = cell_reference(n, H, gh, cp, dc), cell_reference(n, H, gh, cp, dc, torch.float32)
        got = _cell_bwd(x, _dev(ref['c']), n, H, form, fast)
        key, case = f'cell.bwd.n{n}H{H}.fast{fast}', f'gh{int(gh)}cp{int(cp)}dc{int(dc)}'
        _held(key + '.dc_prev', got['dc_prev'], ref['dc_prev'], low['dc_prev'], 1e-5, case)
        if store_dg:
            _held(key + '.dg', got['dg'], ref['dg'], low['dg'], 1e-5, case)
            for g in range(4):              # gate by gate: the f gate's rows are zero without a previous cell, and must be
                sl = slice(g * H, (g + 1) * H)
                if float(ref['dg'][:, sl].abs().max()) == 0.0:
                    assert not bool(got['dg'][:, sl].any())
                else:
                    _held(key + '.dg.gate', got['dg'][:, sl], ref['dg'][:, sl], low['dg'][:, sl], 1e-5, case)
        if n_more is not None:
            more64 = x64['dg_more'][:n_more].sum(0)
            more32 = x64['dg_more'][:n_more].float().sum(0)
            _held(key + '.dgx_sum', got['dgx_sum'], ref['dg'] + more64, low['dg'] + more32, 1e-5, case + f' n_more {n_more}')
            if n_more == 0 and store_dg:
                assert torch.equal(got['dgx_sum'], got['dg'])
        again = _cell_bwd(x, _dev(ref['c']), n, H, form, fast)
        assert all(torch.equal(got[k], again[k]) for k in got)


def test_cell_backward_refuses_more_slabs_without_a_pointer():
    """n_more > 0 with a null dg_more, a negative n_more and an H that is no multiple of 4 are errors, not launches: the outputs
    stay untouched"""
    lib, p, stream = _lib()
    n, H = 3, 8
    x = {k: _dev(v) for k, v in cell_inputs(n, H).items()}
    c = _dev(cell_reference(n, H, False, False, False)['c'])
    dcp, dgx = torch.full((n, H), NAN, device=DEV), torch.full((n, 4 * H), NAN, device=DEV)
    for n_more, more, h_arg in ((1, None, H), (CELL_MORE, None, H), (-1, x['dg_more'], H), (0, None, 6)):
        rc = lib.stove_lstm_cell_bwd(p(x['gx']), None, None, p(c), p(x['dh']), None, None, p(dcp), p(dgx), p(more) if more is not None else None,
                                     n_more, n, h_arg, 1, stream())
        assert rc != 0, (n_more, h_arg)
    assert lib.stove_lstm_cell_fwd(p(x['gx']), None, None, p(dcp), p(dcp), n, 6, 1, stream()) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(dcp).all()) and bool(torch.isnan(dgx).all())


# ------------------------------------------------------------------------------------------------ 2. the network at K = 1 .. 8
def _encoder(K, regime, gemm, arena):
    from stove_amd.arena import ParamArena
    from stove_amd.video_prediction.encoder import RnnStates
    enc = fill_analytic(RnnStates(make_cfg(num_obj=K, encoder_gemm=gemm)), 'sup.encoder.', regime).to(DEV)
    return enc, (ParamArena(enc) if arena else None)


def _pattern(t):
    return (torch.arange(t.numel(), device=t.device, dtype=torch.float32) % 7 + 1).view(t.shape)


@pytest.mark.parametrize('regime', ENC_REGIMES)
@pytest.mark.parametrize('rows', ENC_ROWS)
@pytest.mark.parametrize('K', ENC_COUNTS)
def test_recognition_network_at_every_count(K, rows, regime):
    """codes and the eight parameter gradients under a random output weighting, with the MFMA and the library products, the gradients
    through autograd and (rows % 4 == 0, MFMA products) straight into the arena's views"""
    from stove_amd import ops
    ref, low = encoder_reference(K, rows, regime), encoder_reference(K, rows, regime, torch.float32)
    x64, w64 = encoder_inputs(K, rows)
    x, w = _dev(x64), _dev(w64)
    for gemm in ENC_GEMMS:
        for arena in (True, False):
            enc, ar = _encoder(K, regime, gemm, arena)
            direct = encoder_product_paths(rows, gemm, arena)['direct']
            whh = enc.rnn.weight_hh_l0
            if arena and K == 1:
                with torch.no_grad():
                    whh.grad.copy_(_pattern(whh.grad))
            out = enc(x)
            assert out.shape == (rows, K, 8)
            tag, case = f'enc_counts.K{K}.{regime}.{gemm}', f'rows {rows} arena {int(arena)}'
            _held(tag + '.codes', out, ref['codes'], low['codes'], 1.2e-5, case)
            (out * w).sum().backward()
            torch.cuda.synchronize()
            if arena:
                ar.check()
                assert ops.DIRECT_GRADS and all(id(q) in ops._GRAD_VIEWS for q in enc.parameters())
            for name, p in enc.named_parameters():
                assert p.grad is not None, name
                want, lo = ref['grads'][name], low['grads'][name]
                if K == 1 and name == 'rnn.weight_hh_l0':
                    # no recurrent product runs at one step: exactly zero through autograd, and the arena's slice -- whose semantics
                    # are accumulate -- keeps what it held, on the direct path (never touched) and on autograd's (+ 0)
                    assert not bool(want.any())
                    assert torch.equal(p.grad, _pattern(p.grad) if arena else torch.zeros_like(p.grad)), (gemm, arena, direct)
                    continue
                _held_grad(tag + '.grad', p.grad, want, lo, case + ' ' + name)


@pytest.mark.parametrize('K,rows,regime,gemm', encoder_dx_cases())
def test_encoder_lstm_with_the_gradient_of_its_input(K, rows, regime, gemm):
    """ops.encoder_lstm on its own, time_major=False, x.requires_grad: hidden states, dx and the four LSTM gradients against the
    chained restatement; the parameters are bound to an arena, and the gradient of the input sends them through autograd all the same"""
    from stove_amd import ops
    enc, ar = _encoder(K, regime, gemm, True)
    rnn = enc.rnn
    assert ops.DIRECT_GRADS and all(id(q) in ops._GRAD_VIEWS for q in rnn.parameters())          # bound: direct gradients would be taken
    assert not encoder_product_paths(rows, gemm, True, needs_dx=True)['direct']
    g = torch.Generator().manual_seed(600 + K)
    x64 = torch.rand(rows, 1024, generator=g, dtype=torch.float64).float().double()
    w64 = torch.rand(rows, K, ENC_H, generator=g, dtype=torch.float64).float().double()
    res = {}
    for dtype in (torch.float64, torch.float32):
        _, _, params = oracle_setup(dtype, regime=regime, num_obj=K)
        pr = {k: params['sup.encoder.rnn.' + k] for k in ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0')}
        xa = x64.to(dtype).clone().requires_grad_()
        hs = lstm_chain(xa @ pr['weight_ih_l0'].t() + pr['bias_ih_l0'] + pr['bias_hh_l0'], pr['weight_hh_l0'], K)
        (hs * w64.to(dtype)).sum().backward()
        res[dtype] = {'hs': hs.detach(), 'dx': xa.grad, **{k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in pr.items()}}
    ref, low = res[torch.float64], res[torch.float32]
    x = _dev(x64).requires_grad_()
    hs = ops.encoder_lstm(x, rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0, K, time_major=False, gemm=gemm)
    assert hs.shape == (rows, K, ENC_H)
    tag = f'enc_counts.dx.K{K}.{regime}'
    _held(tag + '.hs', hs, ref['hs'], low['hs'], 1.2e-5)
    (hs * _dev(w64)).sum().backward()
    torch.cuda.synchronize()
    _held_grad(tag + '.grad_x', x.grad, ref['dx'], low['dx'])
    for k in ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0'):
        got = getattr(rnn, k).grad
        if K == 1 and k == 'weight_hh_l0':
            assert not bool(got.any())
        else:
            _held_grad(tag + '.grad', got, ref[k], low[k], k)
    ar.check()


# ------------------------------------------------------------------------------------------------ 3. the reductions of this backward
def _sum_held(key, got, want64, a32, case=''):
    """1e-6, or 6 x the gap of a float32 torch.sum on the CPU"""
    _held(key, got, want64, a32, 1e-6, case)


@pytest.mark.parametrize('cols', COLSUM_COLS)
def test_colsum_against_float64_sums(cols):
    """ops.colsum and stove_colsum2 -- plain, with a second output, and accumulating into both -- at every row count around the
    levels of colsum_level; zero rows give zeros (or leave an accumulating output as it was)"""
    from stove_amd import ops
    lib, p, stream = _lib()
    for rows in COLSUM_ROWS:
        a64 = sum_inputs(rows * 2000 + cols, rows, cols)
        a = _dev(a64)
        want, want32 = a64.sum(0), a64.float().sum(0)
        key, case = f'colsum.c{cols}', f'rows {rows}'
        got = ops.colsum(a)
        assert got.shape == (cols,)
        if rows == 0:
            assert not bool(got.any())
        else:
            _sum_held(key, got, want, want32, case)
        assert torch.equal(got, ops.colsum(a))
        init1, init2 = sum_inputs(7 + cols, cols), sum_inputs(11 + cols, cols) * 3.0
        for acc in (0, 1):
            out1, out2 = _dev(init1).clone(), _dev(init2).clone()
            ws = torch.full((lib.stove_colsum_ws_floats(rows, cols) + 1,), NAN, device=DEV)
            assert lib.stove_colsum2(p(a), p(out1), p(out2), acc, p(ws), rows, cols, stream()) == 0
            torch.cuda.synchronize()
            assert bool(torch.isnan(ws[-1]))                                         # the workspace's stated size is kept
            if rows == 0:
                assert torch.equal(out1, _dev(init1) * acc) and torch.equal(out2, _dev(init2) * acc)
                continue
            _sum_held(key + f'.acc{acc}.out', out1, want + acc * init1, want32 + acc * init1.float(), case)
            _sum_held(key + f'.acc{acc}.out2', out2, want + acc * init2, want32 + acc * init2.float(), case)
            if not acc:
                assert torch.equal(out1, got) and torch.equal(out2, got)             # the same sums in the same order
            again1, again2 = _dev(init1).clone(), _dev(init2).clone()
            assert lib.stove_colsum2(p(a), p(again1), p(again2), acc, p(ws), rows, cols, stream()) == 0
            torch.cuda.synchronize()
            assert torch.equal(out1, again1) and torch.equal(out2, again2)


def test_colsum_refuses_wide_columns_that_are_no_multiple_of_four():
    lib, p, stream = _lib()
    out = torch.full((70,), NAN, device=DEV)
    for cols in (70, 65, 0):
        a = torch.ones(8, max(cols, 1), device=DEV)
        ws = torch.empty(lib.stove_colsum_ws_floats(8, max(cols, 1)) + 1, device=DEV)
        assert lib.stove_colsum2(p(a), p(out), None, 0, p(ws), 8, cols, stream()) != 0, cols
        assert lib.stove_colsum(p(a), p(out), p(ws), 8, cols, stream()) != 0, cols
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


@pytest.mark.parametrize('n', CHUNK_SIZES)
def test_sum_chunks_against_float64_sums(n):
    lib, p, stream = _lib()
    for chunks in CHUNK_COUNTS:
        parts64 = sum_inputs(31 * n + chunks, chunks, n)
        parts = _dev(parts64)
        out = torch.full((n,), NAN, device=DEV)
        assert lib.stove_sum_chunks(p(parts), p(out), n, chunks, stream()) == 0
        torch.cuda.synchronize()
        assert not torch.isnan(out).any()
        _sum_held(f'sum_chunks.n{n}', out, parts64.sum(0), parts64.float().sum(0), f'chunks {chunks}')
        if chunks == 1:
            assert torch.equal(out, parts[0])
        again = torch.full((n,), NAN, device=DEV)
        assert lib.stove_sum_chunks(p(parts), p(again), n, chunks, stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(out, again)
    out = torch.full((8,), NAN, device=DEV)
    for bad_n, bad_chunks in ((6, 2), (7, 1), (8, 0)):
        assert lib.stove_sum_chunks(p(parts), p(out), bad_n, bad_chunks, stream()) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


def test_splitk_weight_gradient_goes_through_sum_chunks():
    """ops._splitk_tn at a row count it splits (2 048 rows: two slices of 1 024) against the float64 product"""
    from stove_amd import ops
    g = torch.Generator().manual_seed(77)
    a64 = (torch.rand(2048, 8, generator=g, dtype=torch.float64) - 0.3).float().double()
    b64 = (torch.rand(2048, 12, generator=g, dtype=torch.float64) - 0.3).float().double()
    got = ops._splitk_tn(_dev(a64), _dev(b64))
    assert got.shape == (8, 12)
    _held('splitk_tn', got, a64.t() @ b64, a64.float().t() @ b64.float(), 1e-6)
    assert torch.equal(got, ops._splitk_tn(_dev(a64), _dev(b64)))
