"""Shared cases of the counter-based start stream's tests (tests/test_env_draw_cpu.py, tests/test_gpu_env_draw.py): the cases, their
specification results (synth.draw_starts_counter, computed once and left unchanged), the call of the CPU driver, and the bit-for-bit
comparison of the five outputs.

Seeds.  A six-ball billiards start is accepted at about 2.3e-4 per attempt, and the kernel tests 64 attempts per round, so the
multibilliards cases are chosen by their `tries` (measured with draw_starts_counter on the CPU; asserted in test_env_draw_cpu.py):
    seed 14: 2 (first round)          seeds 141 .. 145: 1900, 85 (second round), 6053, 864, 54
    seeds 0 .. 4: 2615, 5489, 8293, 6855, 3595 (beyond 4096: dozens of rounds)          seeds 7 .. 11: 2366, 9828, 1895, 1364, 2772
Billiards at seeds 7 .. 11 takes 1, 2, 14, 10, 1 tries, so max_tries = 3 leaves sequences 2 and 3 without a start.

log_pos against np.log on log_grid(): measured maximum 2.0 ulp (of np.log's value; 2.5 ulp against the long-double logarithm), at
x = 0.60951 among others; LOG_ULP_BOUND is that plus one ulp of headroom."""
import functools

import numpy as np

from stove_amd.envs import synth

LOG_ULP_MEASURED, LOG_ULP_BOUND = 2.0, 3.0

ONE_BALL = dict(cls='billiards', n=1, r=1.0, m=1.0, hw=10, granularity=10, res=32, t=1.0, friction_coefficient=0.0, init_v_factor=1.5)
SIX_ACTING = dict(cls='billiards', n=6, r=0.6, m=1.0, hw=10, granularity=10, res=32, t=1.0, friction_coefficient=0.0, init_v_factor=2.0)
GRAVITY_SIX = dict(cls='gravity', n=6, r=2, m=4.0, hw=30, granularity=50, res=32, t=1.0, init_v_factor=0.55, friction_coefficient=0.0)

# name -> (preset, B, T, seed0, max_tries, with_actions)
CASES = {
    'billiards': ('billiards', 5, 12, 7, synth.START_TRIES, None),
    'multibilliards': ('multibilliards', 5, 12, 7, synth.START_TRIES, None),
    'gravity': ('gravity', 5, 12, 7, synth.START_TRIES, None),
    'avoidance': ('avoidance', 5, 12, 7, synth.START_TRIES, None),
    'one_ball_acting': (ONE_BALL, 5, 12, 3, synth.START_TRIES, True),                  # N = 1, a velocity factor, actions
    'six_acting': (SIX_ACTING, 5, 12, 2 ** 40 + 5, synth.START_TRIES, True),           # N = 6 with actions, a seed beyond 32 bits
    'no_start': ('billiards', 5, 12, 7, 3, None),                                      # status [0, 0, 1, 1, 0]
    'gravity_six_last_attempt': (GRAVITY_SIX, 5, 12, 7, 1, None),                      # no attempt is good: attempt 999, status 0
    'multi_first_round': ('multibilliards', 1, 12, 14, synth.START_TRIES, None),
    'multi_second_round': ('multibilliards', 5, 12, 141, synth.START_TRIES, None),
    'multi_many_rounds': ('multibilliards', 5, 12, 0, synth.START_TRIES, None),
}
MULTI_TRIES = {'multi_first_round': [2], 'multi_many_rounds': [2615, 5489, 8293, 6855, 3595]}
OUTPUTS = ('x0', 'v0', 'actions', 'tries', 'status')


@functools.lru_cache(maxsize=None)
def spec_at(name, B=None, T=None):
    """draw_starts_counter on a case, optionally at another B or T -> its dict; shared, so nobody writes into it"""
    preset, b, t, seed0, max_tries, acting = CASES[name]
    out = synth.draw_starts_counter(preset, b if B is None else B, t if T is None else T, seed0, acting, max_tries=max_tries)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def v_factor(name):
    """the kernel's v_factor argument of a case: gravity's factor, billiards' init_v_factor or 0"""
    return float(synth._preset_settings(CASES[name][0], False, None)[3] or 0.0)


def assert_same_bits(got, want, what):
    """the five outputs equal bit for bit (actions: None on both sides or equal)"""
    for k in OUTPUTS:
        g, w = got.get(k), want.get(k)
        if w is None:
            assert g is None, (what, k)
            continue
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), (what, k, g, w)


def log_grid():
    """(0, 1]: 2^-53, the smallest value the uniform can take above 0, and its first multiples; 1 and the doubles just below it;
    geometric and linear sweeps; and the polar method's smallest sums of squares, down to 2^-110"""
    tiny = 2.0 ** -53
    return np.unique(np.concatenate([[tiny, 1.0], np.geomspace(tiny, 1.0, 200001), np.linspace(tiny, 1.0, 100001),
                                     1.0 - tiny * np.arange(1, 2049), tiny * np.arange(1, 2049), np.geomspace(2.0 ** -110, tiny, 20001)]))
