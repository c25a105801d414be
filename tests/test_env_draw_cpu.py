"""CPU-side checks (-m "not gpu") of the counter-based start stream of data synthesis: stove_amd/csrc/env_draw.h -- the text the kernel
of csrc/env_draw.hip runs -- compiled host-only under sanitizers with contraction off (tests/abi/env_draw_driver.cpp) and held to the
numpy specification (stove_amd/envs/synth.py: draw_starts_counter) bit for bit; the header's logarithm against np.log; Philox against
its published vectors; the reference's conditions on every drawn start; the stream's distribution against the host stream's; and the
keyword `starts` through synth_sequences_batched and generate_runs.  The cases are those of tests/env_draw_cases.py."""
import numpy as np
import pytest

import control_harness
import env_draw_cases as C
from stove_amd.envs import synth

KS_BOUND = 1.95 * np.sqrt(2.0 / 4096)          # the 0.1 % critical value of the two-sample statistic at 4096 against 4096: 0.043
CHI2_8_BOUND = 26.124                          # the 0.1 % critical value of chi-square with 8 degrees of freedom
SAMPLES = 4096


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    return control_harness.build_driver(tmp_path_factory, 'env_draw_driver')


def _drive(exe, tmp_path, name):
    preset, B, T, seed0, max_tries, _ = C.CASES[name]
    want = C.spec_at(name)
    s, N, acting = want['settings'], want['settings']['n'], want['actions'] is not None
    ints = np.array([B, N, T, int(acting), int(s['gravity']), max_tries, seed0 & 0xffffffff, seed0 >> 32], dtype=np.uint32).view(np.int32)
    outputs = [('x0', (B, N, 2), np.float64), ('v0', (B, N, 2), np.float64)] + ([('actions', (B, T), np.int32)] if acting else []) + \
              [('tries', (B,), np.int32), ('status', (B,), np.int32)]
    return control_harness.run_driver(exe, tmp_path, ints, [s['hw'], C.v_factor(name)], [want['r']], outputs)


# ------------------------------------------------------------------------------------------------ 1. header = specification, bit for bit
@pytest.mark.parametrize('name', list(C.CASES))
def test_header_equals_the_specification_bit_for_bit(driver, tmp_path, name):
    got, want = _drive(driver, tmp_path, name), C.spec_at(name)
    print(name, 'tries', want['tries'].tolist(), 'status', want['status'].tolist())
    C.assert_same_bits(got, want, name)


def test_the_cases_cover_what_they_are_chosen_for():
    """the status 1 case, gravity's last attempt, the three bands of multibilliards tries, and the settings of every preset"""
    assert C.spec_at('no_start')['status'].tolist() == [0, 0, 1, 1, 0] and C.spec_at('no_start')['tries'].tolist() == [1, 2, 3, 3, 1]
    assert not C.spec_at('no_start')['x0'][2:4].any() and not C.spec_at('no_start')['v0'][2:4].any()
    assert C.spec_at('billiards')['tries'].tolist() == [1, 2, 14, 10, 1]          # (the same attempts, now with room to succeed)
    six = C.spec_at('gravity_six_last_attempt')
    assert six['tries'].tolist() == [1000] * 5 and not six['status'].any() and six['x0'].shape == (5, 6, 2)
    assert C.spec_at('gravity')['tries'].max() < 1000
    for name, tries in C.MULTI_TRIES.items():
        assert C.spec_at(name)['tries'].tolist() == tries
    second = C.spec_at('multi_second_round')['tries']
    assert second[1] == 85 and second[4] == 54
    assert C.spec_at('multi_first_round')['tries'][0] <= 64 < second[1] <= 128 and C.spec_at('multi_many_rounds')['tries'].max() > 4096
    assert C.spec_at('one_ball_acting')['x0'].shape == (5, 1, 2) and C.spec_at('six_acting')['actions'].shape == (5, 12)
    for preset in synth.DATA_NAMES:
        host, counter = synth.draw_starts(preset, 2, 3), synth.draw_starts_counter(preset, 2, 3)
        assert host['settings'] == counter['settings']
        assert np.array_equal(host['r'], counter['r']) and np.array_equal(host['m'], counter['m'])
        assert (counter['actions'] is None) == (host['actions'] is None)
    assert synth.draw_starts('billiards', 2, 3, res=50)['settings'] == synth.draw_starts_counter('billiards', 2, 3, res=50)['settings']
    assert synth.draw_starts_counter('billiards', 0, 3)['x0'].shape == (0, 3, 2)


def test_a_sequence_depends_on_its_seed_alone():
    """sequence i of a batch is sequence 0 of the batch that starts at its seed, whatever the batch and the attempt blocks"""
    whole = C.spec_at('multi_many_rounds')
    for i in (1, 4):
        one = synth.draw_starts_counter('multibilliards', 1, 12, seed0=i)
        C.assert_same_bits({k: one[k] for k in C.OUTPUTS}, {k: (None if whole[k] is None else whole[k][i:i + 1]) for k in C.OUTPUTS}, i)
    acting = C.spec_at('avoidance')
    longer = C.spec_at('avoidance', T=65)
    assert np.array_equal(longer['actions'][:, :12], acting['actions']) and np.array_equal(longer['x0'], acting['x0'])


# ------------------------------------------------------------------------------------------------ 2. the header's logarithm
def test_log_pos_is_the_same_bits_and_within_three_ulp_of_np_log(driver, tmp_path):
    x = C.log_grid()
    assert x.min() == 2.0 ** -110 and x.max() == 1.0 and 2.0 ** -53 in x
    got = control_harness.run_driver(driver, tmp_path, [x.size, 0, 0, 0, 2, 0, 0, 0], [0.0, 0.0], [x], [('log', x.shape, np.float64)])['log']
    spec, ref = synth.log_pos(x), np.log(x)
    assert np.array_equal(got.view(np.int64), spec.view(np.int64))
    at_one = ref == 0.0
    assert at_one.sum() == 1 and spec[at_one][0] == 0.0
    ulp = np.abs(spec[~at_one] - ref[~at_one]) / np.spacing(np.abs(ref[~at_one]))
    print('log_pos against np.log on %d points: at most %.3f ulp' % (x.size, ulp.max()))
    assert ulp.max() <= C.LOG_ULP_BOUND
    assert C.LOG_ULP_BOUND == C.LOG_ULP_MEASURED + 1.0


# ------------------------------------------------------------------------------------------------ 3. Philox and the argument check
def test_philox_known_answers_and_validation_under_sanitizers(driver):
    control_harness.run_modes(driver, ['philox', 'validate'])
    for ctr, key, want in (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
                            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))):
        assert tuple(int(w) for w in synth._philox(*ctr, *key)) == want          # (Random123's kat_vectors, philox4x32 10)
    one = np.uint64(0xffffffff)
    assert synth._uniform(one, one) == 1.0 - 2.0 ** -53 and synth._uniform(np.uint64(31), np.uint64(63)) == 0.0


# ------------------------------------------------------------------------------------------------ 4. the reference's conditions
def _distances(x):
    n = x.shape[1]
    return {(i, j): np.sqrt((x[:, i, 0] - x[:, j, 0]) ** 2 + (x[:, i, 1] - x[:, j, 1]) ** 2) for i in range(n) for j in range(i)}


@pytest.mark.parametrize('name', list(C.CASES))
def test_every_start_meets_the_references_conditions(name):
    st = C.spec_at(name)
    s, ok = st['settings'], st['status'] == 0
    x, v, r, hw = st['x0'][ok], st['v0'][ok], st['r'][ok], s['hw']
    assert ((st['tries'] >= 1) & (st['tries'] <= (1000 if s['gravity'] else C.CASES[name][4]))).all()
    if s['gravity']:
        forced = st['tries'][ok] == 1000
        for d in _distances(x).values():
            assert (d[~forced] > hw / 3).all()
        assert np.isfinite(v).all()
    else:
        assert (x >= r[:, :, None]).all() and (x <= hw - r[:, :, None]).all()
        assert (x - r[:, :, None] >= 0).all() and (x + r[:, :, None] <= hw).all()
        for (i, j), d in _distances(x).items():
            assert (d >= r[:, i] + r[:, j]).all()
        norm = np.sqrt((v ** 2).sum((1, 2)))
        if C.v_factor(name) == 0.0:
            assert (np.abs(norm - 0.5) <= 4 * np.spacing(0.5)).all(), norm
        else:
            f = C.v_factor(name)
            assert ((norm >= 0.5 / f * (1 - 1e-12)) & (norm <= 0.5 * f * (1 + 1e-12))).all()
    if st['actions'] is not None:
        assert st['actions'].dtype == np.int32 and ((st['actions'] >= 0) & (st['actions'] < 9)).all()


# ------------------------------------------------------------------------------------------------ 5. the same distribution as the host's
def _ks(a, b):
    """the two-sample Kolmogorov-Smirnov statistic: the largest distance between the two empirical distribution functions"""
    a, b = np.sort(np.ravel(a)), np.sort(np.ravel(b))
    both = np.concatenate([a, b])
    return float(np.abs(np.searchsorted(a, both, side='right') / a.size - np.searchsorted(b, both, side='right') / b.size).max())


def _run_lengths(actions):
    """the lengths of the runs of equal actions of every row, pooled"""
    out = []
    for row in actions:
        cut = np.flatnonzero(np.diff(row) != 0)
        out.append(np.diff(np.concatenate([[-1], cut, [row.size - 1]])))
    return np.concatenate(out)


@pytest.mark.parametrize('preset', ['billiards', 'gravity', 'avoidance'])
def test_the_stream_has_the_host_streams_distribution(preset):
    """4096 starts of either stream, fixed seeds on both sides: every marginal's two-sample KS statistic stays below the 0.1 % critical
    value (measured when the seeds were fixed: at most 0.0161 over the three presets' marginals, 0.0064 on the run lengths), and so
    does the chi-square of the first action's histogram (measured 9.12)"""
    T = 32
    host, counter = synth.draw_starts(preset, SAMPLES, T, seed0=0), synth.draw_starts_counter(preset, SAMPLES, T, seed0=1 << 33)
    assert not counter['status'].any()
    for key, axis, what in (('x0', 0, 'x'), ('x0', 1, 'y'), ('v0', 0, 'vx'), ('v0', 1, 'vy')):
        d = _ks(host[key][:, :, axis], counter[key][:, :, axis])
        print(preset, what, 'KS %.4f' % d)
        assert d < KS_BOUND, (preset, what, d)
    if preset == 'avoidance':
        d = _ks(_run_lengths(host['actions']), _run_lengths(counter['actions']))
        print(preset, 'run lengths KS %.4f' % d)
        assert d < KS_BOUND
        a, b = (np.bincount(s['actions'][:, 0], minlength=9).astype(np.float64) for s in (host, counter))
        chi2 = float(((a - b) ** 2 / (a + b)).sum())
        print(preset, 'first action chi-square %.2f' % chi2)
        assert chi2 < CHI2_8_BOUND


# ------------------------------------------------------------------------------------------------ 6. synth_sequences_batched(starts=...)
@pytest.mark.parametrize('preset', ['billiards', 'gravity', 'avoidance'])
def test_synth_sequences_batched_on_the_counter_stream(preset):
    host = synth.synth_sequences_batched(preset, 5, 12)
    got = synth.synth_sequences_batched(preset, 5, 12, starts='counter', device=None)
    assert set(got) == set(host)
    for k in host:
        assert got[k].shape == host[k].shape and got[k].dtype == host[k].dtype, k
    assert not np.array_equal(got['y'], host['y'])                                  # (another stream)
    st = synth.draw_starts_counter(preset, 5, 12)
    run = synth.run_starts(st, 12)
    assert np.array_equal(got['y'], run['y']) and np.array_equal(got['X'], run['X']) and np.array_equal(got['in_bounds'], run['in_bounds'])
    assert np.isfinite(got['y']).all() and not np.array_equal(got['y'][:, 0, :, :2], st['x0'])          # (the sequences moved)
    if preset == 'avoidance':
        assert np.array_equal(got['action'].argmax(2)[:, :-1], st['actions'][:, 1:]) and (got['action'].sum(2) == 1).all()
        assert np.array_equal(got['reward'], -run['collisions'].astype(np.float64)[:, :, None])


def test_the_host_stream_is_what_it_was():
    for preset in ('billiards', 'avoidance'):
        st = synth.draw_starts(preset, 4, 6, seed0=3)
        run = synth.run_starts(st, 6)
        for kw in ({}, {'starts': 'host'}):
            got = synth.synth_sequences_batched(preset, 4, 6, seed0=3, **kw)
            assert np.array_equal(got['y'], run['y']) and np.array_equal(got['X'], run['X']) and np.array_equal(got['in_bounds'], run['in_bounds'])
            assert set(got) == ({'X', 'y', 'in_bounds', 'action', 'reward'} if preset == 'avoidance' else {'X', 'y', 'in_bounds'})
    with pytest.raises(ValueError):
        synth.synth_sequences_batched('billiards', 2, 3, starts='device')


# ------------------------------------------------------------------------------------------------ 7. generate_runs(starts='counter')
def test_generate_runs_on_the_counter_stream_counts_missing_starts_as_rejected():
    """billiards from seed 7 with three attempts per start: candidates 2 and 3 (tries 14 and 10) have no start"""
    status = synth.draw_starts_counter('billiards', 12, 6, seed0=7, max_tries=3)['status']
    assert status[:5].tolist() == [0, 0, 1, 1, 0] and (status == 0).sum() >= 5
    want = 7 + np.flatnonzero(status == 0)[:5]
    for chunk in (3, 256):
        data, seeds, bad = synth.generate_runs('billiards', 5, 6, seed0=7, chunk=chunk, filtered=False, starts='counter', start_tries=3)
        assert seeds.tolist() == want.tolist()
        assert bad == int((status[:want[-1] - 7 + 1] != 0).sum()) and bad >= 2
        assert data['y'].shape == (5, 6, 3, 4) and np.isfinite(data['y']).all()
        for i, seed in enumerate(seeds):
            one = synth.synth_sequences_batched('billiards', 1, 6, seed0=int(seed), starts='counter', start_tries=3)
            assert np.array_equal(data['y'][i], one['y'][0]) and np.array_equal(data['X'][i], one['X'][0])
    # the acceptance rule still applies on top: the same candidates as the rule picks from the counter stream's sequences
    full = synth.synth_sequences_batched('gravity', 12, 20, seed0=0, starts='counter')
    good = synth.accepted(full['in_bounds'], 20, 3)
    data, seeds, bad = synth.generate_runs('gravity', 3, 20, seed0=0, chunk=5, starts='counter')
    assert seeds.tolist() == np.flatnonzero(good)[:3].tolist() and bad == int((~good[:seeds[-1] + 1]).sum())
    assert np.array_equal(data['y'], full['y'][seeds])
