"""Long random-shape sweeps over the case generators of tests/fuzz_cases.py (the suite runs a few fixed seeds of each: tests/test_gpu_fuzz.py).
  python tools/fuzz.py FAMILY|all [cases] [first_seed] [--full]
runs seeds first_seed .. first_seed + cases - 1: one line per case (seed, drawn shape and error of the check nearest to its bound), one
more per missed bound, and per family the cases run, the empty ones (draws that are no valid problem) and the worst error per check.
--full draws from the untrimmed choices where a family trims them for the suite.  Exit status 1 if a case misses its bound or more than
20 % of a family's seeds are empty.  A miss does not stop the sweep; any other error does."""
import argparse
import os
import sys

CASES = {'ops': 60, 'fir_march': 120, 'round4': 200, 'round5': 150, 'round5b': 150, 'round6': 120, 'f16': 120}       # default per family
MAX_EMPTY = 0.2


def sweep(family, cases, first_seed, full):
    """True when every case met its bounds and at most MAX_EMPTY of the seeds came back empty."""
    import fuzz_cases
    fn = fuzz_cases.FAMILIES[family][0]
    kw = {'full': True} if full and family in fuzz_cases.FULL else {}
    worst, empty, misses = {}, 0, 0
    for seed in range(first_seed, first_seed + cases):
        results = fn(seed, **kw)
        if not results:
            empty += 1
            print(f'{family} seed={seed} empty', flush=True)
            continue
        what, e, bound, desc = max(results, key=lambda r: r[1] / r[2])                   # (the check nearest to its bound)
        print(f'{family} seed={seed} {what}: {desc}: {e:.3e}', flush=True)
        for what, e, bound, desc in results:
            worst[str(what)] = max(worst.get(str(what), 0.0), e)
            if not e < bound:
                misses += 1
                print(f'{family} seed={seed} MISS {what}: {desc}: {e:.3e} (bound {bound:.0e})', flush=True)
    print(f'{family}: {cases} cases from seed {first_seed}{" (full)" if kw else ""}, {empty} empty, {misses} misses; worst error per check:',
          {k: float(f'{v:.2e}') for k, v in worst.items()}, flush=True)
    if empty > MAX_EMPTY * cases:
        print(f'{family}: more than {MAX_EMPTY:.0%} of the seeds are empty: the sweep covers less than it claims', flush=True)
    return not misses and empty <= MAX_EMPTY * cases


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('family', choices=list(CASES) + ['all'])
    ap.add_argument('cases', type=int, nargs='?', help='per family; default: ' + ', '.join(f'{k} {v}' for k, v in CASES.items()))
    ap.add_argument('first_seed', type=int, nargs='?', default=0)
    ap.add_argument('--full', action='store_true')
    a = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, 'tests')]
    import torch
    with torch.no_grad():                   # (as the suite runs them: tests/conftest.py; a case that needs gradients switches them on)
        ok = [sweep(f, CASES[f] if a.cases is None else a.cases, a.first_seed, a.full) for f in (CASES if a.family == 'all' else [a.family])]
    sys.exit(0 if all(ok) else 1)


if __name__ == '__main__':
    main()
