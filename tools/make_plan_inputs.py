"""Choose the 'spread' factors and input seeds of tests/plan_cases.py and write tests/golden/plan_counts_inputs.npz.

    python tools/make_plan_inputs.py tune      # prints SPREAD_K / INPUT_SEEDS / SEARCH_SPREAD_K / RH_SPREAD_K / search seeds to paste into plan_cases.py
    python tools/make_plan_inputs.py write     # draws every case's inputs with the tables as committed and writes the fixture

tune, per expansion case: for seed 0, 1, ... the case's plain draws (nothing passed over) are scored at k = 1 .. 4 in steps of 1/16;
the middle of the longest run of k at which the three conditions of the 'spread' fill hold is taken, the inputs are drawn at that k
with the ReLU margin enforced, and the conditions are asserted on them -- else the seed is passed over.  CPU only, float64."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tests', 'golden')):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch                # noqa: E402

import plan_cases as P      # noqa: E402

K_GRID = [1.0 + i / 16 for i in range(49)]


def longest_run_middle(good):
    """good: list of bool over K_GRID -> the k in the middle of the longest run of True, or None"""
    best, start = None, None
    for i, g in enumerate(list(good) + [False]):
        if g and start is None:
            start = i
        if not g and start is not None:
            if best is None or i - start > best[1] - best[0]:
                best = (start, i)
            start = None
    return None if best is None else K_GRID[(best[0] + best[1] - 1) // 2]


def tune_expansion(case, seeds=range(60)):
    for seed in seeds:
        P.INPUT_SEEDS[(case.name, 'spread')] = seed
        P.SPREAD_K[case.name] = 1.0
        z, app, acts, _ = P.make_inputs(case, 'spread', reject=False)
        good = [P.spread_conditions(*P.preacts_of(case, ('scaled', k), z, app, acts))[0] for k in K_GRID]
        k = longest_run_middle(good)
        if k is None:
            continue
        P.SPREAD_K[case.name] = k
        z, app, acts, redrawn = P.make_inputs(case, 'spread')
        ok, fig = P.spread_conditions(*P.preacts_of(case, ('scaled', k), z, app, acts))
        if ok:
            return seed, k, fig, redrawn
    return None


def tune_search(s, seeds=range(60)):
    """-> (seed, k, smallest decision gap, seeds passed over): the conditions of the fill on the rewards of the search's own expansions
    are scored on a plain expansion of the roots"""
    case = P._case('search', s.N, s.A, s.app, s.M, 2 * s.D, s.D)
    passed = []
    for seed in seeds:
        cand = s._replace(seed=seed)
        z, app, acts = P.search_inputs(cand)
        good = [P.spread_conditions(*P.preacts_of(case, ('scaled', k), z, app, torch.from_numpy(acts[0])))[0] for k in K_GRID]
        k = longest_run_middle(good)
        if k is not None:
            P.SEARCH_SPREAD_K[P.search_id(s)] = k
            f, _ = P.search_on_oracle(cand)
            if f.min_gap >= P.SEARCH_GAP:
                return seed, k, f.min_gap, passed
        passed.append(seed)
    raise SystemExit('no seed for search ' + P.search_id(s))


def tune_rh(N):
    """k of the reward-head cases at N objects: scored on the 1 025-item case, the items without a planted entry"""
    good = []
    for k in K_GRID:
        P.RH_SPREAD_K[N] = k
        P.rh_params.cache_clear()
        P.rh_inputs.cache_clear()
        good.append(P.rh_spread_conditions(N)[0])
    k = longest_run_middle(good)
    if k is None:
        raise SystemExit('no k for the reward head at N = %d' % N)
    P.RH_SPREAD_K[N] = k
    P.rh_params.cache_clear()
    P.rh_inputs.cache_clear()
    return k, P.rh_spread_conditions(N)[1]


def tune(only):
    for N in range(1, 9) if not only else ():
        k, fig = tune_rh(N)
        print('RH_SPREAD_K[%d] = %r   # %s' % (N, k, fig), flush=True)
    for case in P.expansion_cases():
        if only and not any(o in case.name for o in only):
            continue
        found = tune_expansion(case)
        if found is None:
            print('NO SEED', case.name, flush=True)
            continue
        seed, k, fig, redrawn = found
        print('SPREAD_K[%r] = %r; INPUT_SEEDS[(%r, "spread")] = %d   # %s redrawn %s' % (case.name, k, case.name, seed, fig, redrawn), flush=True)
    for s in P.SEARCH_CASES if (not only or 'search' in only) else ():
        seed, k, gap, passed = tune_search(s)
        print('search %s: seed %d k %r gap %.3g passed over %s' % (P.search_id(s), seed, k, gap, passed), flush=True)


if __name__ == '__main__':
    if sys.argv[1:2] == ['tune']:
        tune(sys.argv[2:])
    elif sys.argv[1:] == ['write']:
        P.write_fixture()
    else:
        raise SystemExit(__doc__)
