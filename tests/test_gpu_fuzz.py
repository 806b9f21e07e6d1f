"""Seeded random-shape cases of the fuzz families, as a bounded part of the suite (run with -m gpu on an MI355X).

Every family of tests/fuzz_cases.py draws a fixed number of cases from fixed seeds, one test per case, against the family's own error bound.
A failure names the family, the seed and the drawn shape; ``python tools/fuzz.py FAMILY 1 SEED`` reproduces it, and the same driver runs the
long sweeps over other seeds."""
import pytest

from fuzz_cases import FAMILIES

pytestmark = pytest.mark.gpu


def _check(family, seed, results):
    """results: list of (what, error, bound, description)."""
    worst = max((e for _, e, _, _ in results), default=0.0)
    print(f'FUZZ {family} seed={seed} worst={worst:.3e}')
    bad = [f'{what}: {desc}: {e:.3e} (bound {b:.0e})' for what, e, b, desc in results if not e < b]
    assert not bad, f'{family} seed {seed}: ' + '; '.join(bad)


@pytest.mark.parametrize('family,seed', [(f, s0 + k) for f, (_, s0, n) in FAMILIES.items() for k in range(n)])
def test_fuzz(family, seed):
    _check(family, seed, FAMILIES[family][0](seed))
