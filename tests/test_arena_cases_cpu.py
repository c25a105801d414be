"""tests/arena_cases.py without a GPU: the float64 references of the arena, optimiser, input and noise kernels are pinned to
something that does not share their code (torch.distributions, torch.optim.Adam, the published Philox answers, the model's own
parameter image), and every condition the cases of tests/test_gpu_arena_kernels.py rely on is asserted -- for every case; none is
skipped.  The float32 gaps of the references (what the bars of the GPU file are made from) are printed."""
import math

import numpy as np
import pytest
import torch

import arena_cases as A
from gpu_helpers import regime_bar


# ------------------------------------------------------------------------------------------------------------------ 1. table bake
def _float64_supair(fill):
    from stove_amd.video_prediction.supair import Supair
    src = A.bake_model('supair', fill)[1]
    sup = Supair(A.model_cfg(torch.float64)).double()
    sup.load_state_dict({k: v.detach().double() for k, v in src.state_dict().items()})
    return sup


def _variance(leaf, args):
    return args.gauss_min_sigma + (args.gauss_max_sigma - args.gauss_min_sigma) * torch.sigmoid(leaf.sigma_params)


@pytest.mark.parametrize('fill', A.BAKE_FILLS)
def test_bake_reference_is_the_normal_log_density_and_a_softmax(fill):
    """a x^2 + b x + c = Normal(mu, sqrt(var)).log_prob(x) in float64 at random x for every leaf entry of both SPNs, found through the
    SPN's own structure (root -> product -> sum -> product -> leaf, pixel by pixel through the leaves' scopes), not through the index
    plans; every softmax column sums to 1; the reference is float64 and gives 74 parameter gradients."""
    from torch.distributions import Normal
    sup = _float64_supair(fill)
    ref = A.bake_reference(fill)
    assert all(t.dtype == torch.float64 for t in ref['tables']) and [t.numel() for t in ref['tables']] == list(A.TABLE_FLOATS)
    assert len(ref['grads']) == 74 and all(g.dtype == torch.float64 and torch.isfinite(g).all() for g in ref['grads'].values())
    oc, ow, orr, bc, bw = [t.view(s) for t, s in zip(ref['tables'], ((24, 25, 10, 3), (12, 100, 10), (6, 100), (3, 1024, 6, 3), (3, 36)))]
    g = torch.Generator().manual_seed(1)
    obj, bg = sup.obj_spn, sup.bg_spn
    q = 0
    for prod in obj.output_vector.inputs:
        for s in prod.inputs:
            for leaf in s.inputs[0].inputs:
                x = torch.rand(25, 10, generator=g, dtype=torch.float64) * 1.4 - 0.2
                want = Normal(leaf.means, torch.sqrt(_variance(leaf, obj.args))).log_prob(x)
                got = oc[q, ..., 0] * x * x + oc[q, ..., 1] * x + oc[q, ..., 2]
                assert float(((got - want).abs() / (1.0 + want.abs())).max().detach()) < 1e-12, (fill, q)
                q += 1
    assert q == 24
    seen = torch.zeros(3, 1024, dtype=torch.bool)
    for r, prod in enumerate(bg.output_vector.inputs):
        for leaf in prod.inputs:
            px = torch.tensor(leaf.scope)
            x = torch.rand(len(px), 6, generator=g, dtype=torch.float64) * 1.4 - 0.2
            want = Normal(leaf.means, torch.sqrt(_variance(leaf, bg.args))).log_prob(x)
            c = bc[r, px]
            got = c[..., 0] * x * x + c[..., 1] * x + c[..., 2]
            assert float(((got - want).abs() / (1.0 + want.abs())).max().detach()) < 1e-12, (fill, r)
            seen[r, px] = True
    assert bool(seen.all())
    assert float((ow.sum(1) - 1.0).abs().max()) < 1e-12 and abs(float(orr.sum()) - 1.0) < 1e-12 and abs(float(bw.sum()) - 1.0) < 1e-12
    assert float(ow.min()) > 0.0 or fill == 'edges'


@pytest.mark.parametrize('fill', A.BAKE_FILLS)
def test_bake_tables_do_not_depend_on_what_surrounds_the_supair(fill):
    """the tables of a bare Supair and of the Supair inside a Stove are identical, so one reference serves both arenas; the two
    arenas differ in what surrounds the SPN tensors, and both index plans name the same 74 tensors"""
    (_, sup_a, ar_a), (_, sup_b, ar_b) = A.bake_model('supair', fill), A.bake_model('stove', fill)
    for a, b in zip(A.tables_of(sup_a), A.tables_of(sup_b)):
        assert torch.equal(a, b)
    sa, sb = A.spn_spans('supair', fill), A.spn_spans('stove', fill)
    assert list(sa) == list(sb) == list(A.bake_reference(fill)['grads']) and len(sa) == 74
    assert ar_b.numel > ar_a.numel and len(ar_b.params) == 162 and len(ar_a.params) == 82
    for model, spans, ar in (('supair', sa, ar_a), ('stove', sb, ar_b)):
        outside = A.outside_mask(model, fill)
        assert outside.sum() == ar.numel - sum(k for _, k in spans.values())
        assert outside[:min(o for o, _ in spans.values())].all() and outside.sum() > 30000          # other parameters in front
        pads = sum((-k) % 4 for _, k in spans.values())
        assert pads > 0                                    # alignment pads between the SPN's own tensors
        pat = A.bake_pattern(model, fill)
        assert pat.dtype == np.float32 and (pat != 0).all() and np.isfinite(pat).all()


def test_planted_edges_are_what_they_claim():
    sup = A.bake_model('supair', 'edges')[1]
    obj, bg = sup.obj_spn, sup.bg_spn
    for spn in (obj, bg):
        rho = torch.cat([v.sigma_params.reshape(-1) for v in spn.vector_list[0]]).detach()
        for v in (30.0, -30.0, 100.0, -100.0):
            assert int((rho == v).sum()) >= 4
        s = torch.sigmoid(rho[(rho == 30.0) | (rho.abs() == 100.0)])
        assert bool(((s * (1 - s)) == 0).all())                                     # s (1 - s) = 0 in float32 (9.4e-14 at -30)
        assert math.isinf(float(torch.exp(torch.tensor(100.0))))                    # expf(100) overflows
        var = spn.args.gauss_min_sigma + (spn.args.gauss_max_sigma - spn.args.gauss_min_sigma) * torch.sigmoid(rho[rho.abs() == 100.0])
        lo, hi = spn.args.gauss_min_sigma, spn.args.gauss_max_sigma                  # at a bound, to the float32 rounding of lo + (hi - lo)
        assert len(set(var.tolist())) == 2 and all(min(abs(x - lo), abs(x - hi)) <= 1.5e-8 for x in var.tolist())
    sums = list(obj.vector_list[2])
    assert float(sums[0].params[:, 0].detach().std()) == 0.0 and float(sums[5].params[:, 9].detach().std()) == 0.0
    for node, col, row in ((1, 3, 17), (11, 0, 99)):
        c = sums[node].params[:, col].detach()
        assert float(c[row] - torch.cat([c[:row], c[row + 1:]]).max()) == 90.0
    ref = A.bake_reference('edges')
    ow = ref['tables'][1].view(12, 100, 10)
    so = obj._plan_cpu['sum_order'].tolist()
    assert float((ow[so.index(0)][:, 0] - 0.01).abs().max()) < 1e-15
    assert float(ow[so.index(1)][17, 3]) == 1.0 and 0 < float(ow[so.index(1)][0, 3]) < 1e-38          # e^-90: below float32's normal range
    plain = A.bake_reference('analytic')
    assert float(ref['tables'][2].max()) > 4 * float(plain['tables'][2].max()) and float(ref['tables'][2].min()) < 1e-15      # root x 20
    assert 3e-19 < float(A.bake_reference('stress')['tables'][1].min()) < 6e-19       # the smallest 'stress' sum weight: 4e-19


def test_bake_gaps_lie_within_their_caps():
    """the float32 gaps of the reference, per quantity the largest over the four fills: printed, and each within twice the value
    arena_cases.BAKE_MEASURED records (so no gap can grow a bar unnoticed); how many bars the gap rule sets"""
    worst, by_gap, total = {k: (0.0, None) for k in A.BAKE_BASE}, 0, 0
    for fill in A.BAKE_FILLS:
        for key, gaps in A.bake_gaps(fill).items():
            for name, gap in gaps.items():
                total += 1
                by_gap += regime_bar(A.BAKE_BASE[key], gap) > A.BAKE_BASE[key]
                if gap > worst[key][0]:
                    worst[key] = (gap, '%s / %s' % (fill, name))
    for key, (gap, where) in worst.items():
        print('largest float32 gap of %-15s %.3g (%s; recorded %.3g)' % (key, gap, where, A.BAKE_MEASURED[key]))
        assert 0.25 * A.BAKE_MEASURED[key] <= gap <= 2.0 * A.BAKE_MEASURED[key], (key, gap)     # the record is a measurement, the cap twice it
    print('the gap rule sets %d of %d bars' % (by_gap, total))
    # the upstream gradients reach every tensor: no reference gradient is zero, and the pattern under it is far above the bars
    for fill in A.BAKE_FILLS:
        for n, g in A.bake_reference(fill)['grads'].items():
            assert float(g.abs().max()) > 0, (fill, n)
    assert A.PATTERN_SHIFT > 10 * regime_bar(A.BAKE_BASE['grad'], A.BAKE_MEASURED['grad'])         # an overwrite is 10 x the largest bar off
    assert A.PATTERN_SHIFT * 2.0 ** -24 / 1e-3 < 0.05 * A.BAKE_BASE['grad.small']                  # and its rounding far below the smallest


# ------------------------------------------------------------------------------------------------------------------ 2. gather / scatter
@pytest.mark.parametrize('cl,ac', A.GNN_CASES)
def test_gnn_tables_name_every_float_once_and_only_gnn_parameters(cl, ac):
    from stove_amd import ops
    dyn, arena = A.gnn_case(cl, ac)
    inside = np.zeros(arena.numel, dtype=bool)
    for p in arena._gnn_params:
        o = arena.offset[id(p)]
        inside[o:o + p.numel()] = True
    assert 0 < inside.sum() < arena.numel
    for k in range(3):
        src, src_g = (t.numpy() for t in arena._gnn[k])
        w, v, wt = dyn.param_image(k)
        assert src_g.size == w.numel() + v.numel() and src.dtype == np.int32 and src_g.dtype == np.int32
        for t in (src, src_g):
            live = t[t >= 0]
            assert live.size and live.max() < arena.numel and inside[live].all()
            assert (t < 0).any() or cl == 32                    # pads of the image: gathered as zero, never scattered
        live = src_g[src_g >= 0]
        assert np.unique(live).size == live.size            # the scatter's `+=` is not atomic: no arena float twice
        want = ops.gnn_width(cl).layout(w, v, wt).detach().numpy()
        assert np.array_equal(A.gather_reference(arena.data.numpy(), src), want)
        # the scatter's reference puts every gradient entry where the parameter lives
        g = A.pattern(src_g.size, seed=k)
        out = A.scatter_reference(np.zeros(arena.numel, np.float32), src_g, g)
        assert np.array_equal(out[live], g[src_g >= 0]) and not out[~inside].any()


def test_synthetic_tables():
    for n in A.SYNTH_N:
        gat, sca = A.synth_tables(n)
        assert gat.size == sca.size == n
        live = sca[sca >= 0]
        assert np.unique(live).size == live.size and (live.size == 0 or live.max() < A.SYNTH_ARENA)
        if n >= 255:
            assert (gat < 0).any() and (sca < 0).any() and np.unique(gat[gat >= 0]).size < (gat >= 0).sum()
    assert A.SYNTH_N == (0, 1, 255, 256, 257)


# ------------------------------------------------------------------------------------------------------------------ 3. FlatAdam
@pytest.mark.parametrize('amsgrad', [True, False])
def test_adam_reference_is_torch_adam_in_float64(amsgrad):
    """five steps, a new learning rate and new gradients each, clipping on: adam_reference against torch.optim.Adam +
    clip_grad_norm_ in float64 to 1e-12.  Tensor 1 receives no gradient until step 3 (its own step count), tensor 2 is frozen: it
    is in the clipped norm but not in the optimiser."""
    rs = np.random.RandomState(3)
    sizes = (5, 18, 7, 33)
    segs, off = [], 0
    for k in sizes:
        segs.append((off, k, 'train'))
        off += (k + 3) // 4 * 4
    trainable = np.array([1, 1, 0, 1], np.uint8)
    st = {'p': np.zeros(off), 'm': np.zeros(off), 'v': np.zeros(off), 'vmax': np.zeros(off) if amsgrad else None, 'steps': np.zeros(4)}
    for (o, k, _) in segs:
        st['p'][o:o + k] = rs.standard_normal(k)
    params = [torch.nn.Parameter(torch.from_numpy(st['p'][o:o + k].copy())) for o, k, _ in segs]
    opt = torch.optim.Adam([params[0], params[1], params[3]], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, amsgrad=amsgrad)
    for step in range(5):
        lr = 1e-3 * 0.8 ** step
        g = np.zeros(off)
        for i, (o, k, _) in enumerate(segs):
            if not (i == 1 and step < 2):
                g[o:o + k] = rs.standard_normal(k) * (1.0 + i)
        for i, (o, k, _) in enumerate(segs):
            params[i].grad = None if (i == 1 and step < 2) else torch.from_numpy(g[o:o + k].copy())
        max_norm = 0.7 * A.grad_norm64(g) if step % 2 == 0 else 3.0 * A.grad_norm64(g)
        tn = torch.nn.utils.clip_grad_norm_(params, max_norm)
        opt.param_groups[0]['lr'] = lr
        opt.step()
        r = A.adam_reference(st['p'], g, st['m'], st['v'], st['vmax'], segs, trainable, st['steps'], (lr, 0.9, 0.999, 1e-8), max_norm)
        st.update({k: r[k] for k in ('p', 'm', 'v', 'vmax', 'steps')})
        assert abs(r['norm'] - float(tn)) < 1e-12 * float(tn)
        for i, (o, k, _) in enumerate(segs):
            assert float(np.abs(st['p'][o:o + k] - params[i].detach().numpy()).max()) < 1e-12, (step, i)
            if i != 2 and i in [j for j, q in enumerate(params) if q in opt.state]:
                s = opt.state[params[i]]
                assert float(s['step']) == st['steps'][i]
                assert float(np.abs(st['m'][o:o + k] - s['exp_avg'].numpy()).max()) < 1e-12
                assert float(np.abs(st['v'][o:o + k] - s['exp_avg_sq'].numpy()).max()) < 1e-12 * max(1.0, float(s['exp_avg_sq'].max()))
                if amsgrad:
                    assert float(np.abs(st['vmax'][o:o + k] - s['max_exp_avg_sq'].numpy()).max()) < 1e-12 * max(1.0, float(s['max_exp_avg_sq'].max()))
    assert st['steps'].tolist() == [5.0, 3.0, 0.0, 5.0]
    o, k, _ = segs[2]
    assert np.array_equal(st['p'][o:o + k], params[2].detach().numpy()) and not st['m'][o:o + k].any()


def test_adam_sizes_reach_every_path_of_the_three_kernels():
    assert A.SCAN_SPAN == 262144 and A.ADAM_SIZES['n1024'] == 1024 and A.ADAM_SIZES['n262144'] == A.SCAN_SPAN
    assert A.ADAM_SIZES['n262148'] == A.SCAN_SPAN + 4                    # one scan thread takes a second trip,
    o, k, kind = A.adam_segments('n262148')[0][-1]                       # and only there is the last segment's one gradient entry
    assert kind == 'last' and (o + k - 1) // 4 == A.SCAN_SPAN // 4 and A.adam_case('n262148', 'unit', True)['g'][o + k - 1] != 0
    from stove_amd.arena import ParamArena
    from stove_amd.video_prediction.stove import Stove
    segs, numel = A.adam_segments('stove')
    arena = ParamArena(Stove(A.model_cfg()), world_size=1)
    assert len(segs) == 162 and numel == arena.numel and 1.4e6 < numel < 1.5e6 and numel > 5 * A.SCAN_SPAN
    assert [o for o, _, _ in segs] == [arena.offset[id(p)] for p in arena.params]
    assert sum(1 for o, _, _ in segs if o % 1024) > 100                  # update blocks (1024 floats) straddle segments
    for size in A.ADAM_SIZES:
        segs, numel = A.adam_segments(size)
        assert numel % 4 == 0 and (A.ADAM_SIZES[size] in (None, numel))
        for (o, k, kind), (o2, _, _) in zip(segs, segs[1:] + [(numel, 0, '')]):
            assert o % 4 == 0 and o + k <= o2 < o + k + 4
        kinds = {kind for _, _, kind in segs}
        assert kinds == set(A.KINDS) if numel >= 1024 else kinds == {'last'}
        for o, k, kind in segs:
            assert kind != 'last' or k % 4 != 0                             # its last float shares a float4 with pad zeros


@pytest.mark.parametrize('case', A.ADAM_CASES, ids=A.adam_id)
def test_adam_case_conditions(case):
    size, clip, family, amsgrad = case
    c = A.adam_case(size, family, amsgrad)
    segs, g, v = c['segs'], c['g'], c['v']
    norm = A.grad_norm64(g)
    big = c['numel'] >= 1024
    seen_steps, seen_scales = set(), set()
    for i, (o, k, kind) in enumerate(segs):
        hi = o + (k + 3) // 4 * 4
        gs = g[o:o + k]
        assert not g[o + k:hi].any() and not c['m'][o + k:hi].any() and not v[o + k:hi].any()        # pads: zero where the update reads them
        assert (c['p'][o + k:hi] == 7.0).all()
        assert (c['m'][o:o + k] != 0).all() and (v[o:o + k] > 0).all()
        if kind in ('train', 'frozen'):
            assert (gs != 0).all()
        elif kind == 'last':
            assert gs[-1] != 0 and not gs[:-1].any() and hi > o + k
        else:
            assert not gs.any()
        assert bool(c['trainable'][i]) == (kind in ('train', 'train_zero', 'last'))
        if kind in ('train', 'last'):
            seen_steps.add(float(c['steps'][i]))
            seen_scales.add(float(np.abs(gs).max()) > 1e3 and 1e6 or float(np.abs(gs).max()) < 1e-6 and 1e-12 or 1.0)
            if float(np.abs(gs).max()) < 1e-6:
                assert float(np.sqrt(v[o:o + k]).max()) < A.HYPER[3]                               # sqrt(v) below eps
        if amsgrad:
            x = c['vmax'][o:o + k]
            assert (x[0::2] > v[o:o + k][0::2]).all() and (k < 2 or (x[1::2] < v[o:o + k][1::2]).all())
            assert (c['vmax'][o + k:hi] == 3.0).all()
        if family == 'zero':
            assert not c['p'][o:o + k].any()
        else:
            assert float(np.abs(c['p'][o:o + k]).min()) >= 0.25 and float(np.abs(c['p'][o:o + k]).max()) <= 1.25
    if big:
        assert seen_steps == set(A.STEPS_IN) and seen_scales == set(A.GRAD_SCALES), (seen_steps, seen_scales)
    mn = A.max_norm_of(c, clip)
    if clip != 'off':
        assert abs(mn / (norm + 1e-6) - 1.0) > 1e-3                       # no float32 norm can flip the clamp
        n32 = float(np.float32(norm))
        for wobble in (1 - 1e-4, 1.0, 1 + 1e-4):                          # whatever float32 sum the device forms
            coef = min(np.float32(1.0), np.float32(mn) / (np.float32(n32 * wobble) + np.float32(1e-6)))
            assert (coef == 1.0) == (clip == 'twice')
    hi64, lo32 = A.adam_expected(*case), A.adam_expected(*case, np.float32)
    if clip == 'twice':
        for ref, dt in ((hi64, np.float64), (lo32, np.float32)):
            off = A.adam_expected(size, 'off', family, amsgrad, dt)
            for k in ('p', 'm', 'v', 'vmax'):
                assert (ref[k] is None and off[k] is None) or np.array_equal(ref[k], off[k])
    # what steps and what stays
    for i, (o, k, kind) in enumerate(segs):
        assert bool(hi64['active'][i]) == (kind in ('train', 'last'))
        assert hi64['steps'][i] == c['steps'][i] + (1.0 if hi64['active'][i] else 0.0)
        if not hi64['active'][i]:
            for key in ('p', 'm', 'v'):
                assert np.array_equal(hi64[key][o:o + k], c[key][o:o + k].astype(np.float64))
        else:
            assert (hi64['p'][o:o + k] != c['p'][o:o + k]).all()
    gaps = A.adam_gaps(*case)
    print(A.adam_id(case), ' '.join('%s %.3g' % kv for kv in sorted(gaps.items())))
    assert all(np.isfinite(x) and x < 1e-4 for x in gaps.values()), gaps            # a gap beyond that would make the 6 x bar meaningless


def test_adam_strict_zero_reference_over_two_calls():
    """a gradient, then zeros: with the sticky bit the segments that stepped step again on their momentum, without it nothing moves"""
    c = A.adam_case(A.STRICT_ZERO_SIZE, 'unit', True)
    assert c['numel'] > 1024
    for sticky in (False, True):
        first, second = A.adam_two_calls(sticky)
        assert first['active'].any() and not first['active'].all()
        assert second['active'].tolist() == (first['active'].tolist() if sticky else [False] * len(c['segs']))
        assert np.array_equal(second['p'], first['p']) != sticky
        assert np.array_equal(second['steps'], first['steps'] + (first['active'] if sticky else 0))
        assert np.array_equal(first['flags'], first['active'] | (np.array([k == 'frozen' for _, _, k in c['segs']]))) if sticky else not first['flags'].any()
    gaps = A.adam_two_calls_gaps()
    print('strict_zero', ' '.join('%s %.3g' % kv for kv in sorted(gaps.items())))
    assert all(np.isfinite(x) and x < 1e-4 for x in gaps.values()), gaps


# ------------------------------------------------------------------------------------------------------------------ 4. bw_transform
@pytest.mark.parametrize('C,P,N', A.BW_SHAPES)
def test_bw_inputs_make_the_clamp_act_on_both_sides(C, P, N):
    assert P % 4 == 0 and (P != 2500 or (P // 4) % 256 != 0)                 # at 2 500 pixels frames straddle the 256-thread blocks
    for u8 in (False, True):
        x = A.bw_inputs(C, P, N, u8)
        assert x.shape == (N, C, P) and x.dtype == (torch.uint8 if u8 else torch.float32)
        s = A.bw_sums(x)
        ref = A.bw_reference(x)
        assert ref.dtype == torch.float32 and ref.shape == (N, P) and float(ref.min()) == 0.0 and float(ref.max()) == 1.0
        if u8 and C == 1:
            assert float((s == 1.0).double().mean()) >= 0.1                  # one channel of x / 255 cannot exceed 1: a tenth sit at 1
        else:
            assert float((s > 1.0).double().mean()) >= 0.1
        if not u8:
            assert bool((s < 0.0).any())
        assert bool((s == 0.0).any()) and bool((s == 1.0).any())
        assert bool(((s > 0.0) & (s < 1.0)).any()) or P == 4
        # the float32 reference against the float64 value of the same formula
        d = float((ref.double() - s.clamp(0.0, 1.0)).abs().max())
        assert d <= 1.2e-7, (C, P, N, u8, d)


# ------------------------------------------------------------------------------------------------------------------ 5. noise
def test_philox_known_answers():
    for ctr, key, want in A.PHILOX_KAT:
        got = A.philox4x32_10([np.array([c]) for c in ctr], [np.array([k]) for k in key])
        assert tuple(int(w[0]) for w in got) == want
    # vectorised over the counter like noise_reference uses it
    got = A.philox4x32_10((np.zeros(3), np.zeros(3), np.arange(3), np.zeros(3)), (np.zeros(3), np.zeros(3)))
    assert tuple(int(w[0]) for w in got) == A.PHILOX_KAT[0][2] and len({int(w) for w in got[0]}) == 3


def test_noise_reference():
    assert A.NOISE_N == (1, 3, 4, 5, 1023, 1024, 1025, 262147) and A.noise_bar() <= A.NOISE_CAP == 1e-4
    assert A.NOISE_STATES['zero'] == (0, 0) and A.NOISE_STATES['seed_max'][0] == 2 ** 64 - 1
    assert A.NOISE_STATES['call_hi'][1] == 2 ** 32 and A.NOISE_STATES['call_max'][1] == 2 ** 64 - 1
    # thread 0 of state (0, 0) is the first known answer
    c = [w / 2.0 ** 32 for w in A.PHILOX_KAT[0][2]]
    u = [((w >> 8) + 0.5) / 2.0 ** 24 for w in A.PHILOX_KAT[0][2]]
    r0, r1 = math.sqrt(-2 * math.log(u[0])), math.sqrt(-2 * math.log(u[2]))
    want = [r0 * math.cos(2 * math.pi * u[1]), r0 * math.sin(2 * math.pi * u[1]), r1 * math.cos(2 * math.pi * u[3]), r1 * math.sin(2 * math.pi * u[3])]
    assert np.allclose(A.noise_reference(0, 0, 4), want, rtol=0, atol=1e-14) and len(c) == 4
    for name, (seed, call) in A.NOISE_STATES.items():
        big = A.noise_reference(seed, call, 262147)
        assert big.shape == (262147,) and np.isfinite(big).all()
        assert abs(big.mean()) < 8e-3 and abs(big.var() - 1.0) < 1.5e-2 and 4.0 < np.abs(big).max() < 6.0
        for n in A.NOISE_N:
            assert np.array_equal(A.noise_reference(seed, call, n), big[:n])          # a draw depends on (seed, call, element) only
    # every word of the state matters
    base = A.noise_reference(5, 7, 64)
    for seed, call in ((5 + 2 ** 32, 7), (5, 7 + 2 ** 32), (6, 7), (5, 8)):
        assert np.abs(A.noise_reference(seed, call, 64) - base).max() > 0.5
