"""The float64 reference, the merge rule, the derived bound and the float32 kernel model of tests/token_entropy_refs.py (no GPU):
the reference has the properties the definition promises, the merge rule equals the direct evaluation, the model of the kernels'
arithmetic stays inside the bound on crafted rows, and two planted faults leave it -- so the bound discriminates."""
import numpy as np
import pytest

from tests import token_entropy_refs as R

V_TINY = 333            # V % 4 != 0: one pad column at least
V_LARGE = 51866


def test_reference_properties():
    for V in (7, V_TINY):
        x = np.full(V + 3, 1.25, np.float32)
        assert abs(R.reference(x, V) - np.log(V)) < 1e-12                    # all equal: log V, the pad columns excluded
        x[V:] = 75.0
        assert abs(R.reference(x, V) - np.log(V)) < 1e-12
        one = np.full(V, -np.inf, np.float32); one[V // 2] = -3.5
        assert R.reference(one, V) == 0.0                                    # a single finite logit: exactly 0
        two = one.copy(); two[0] = -3.5
        assert abs(R.reference(two, V) - np.log(2)) < 1e-12                  # -inf columns are ignored
        assert np.isnan(R.reference(np.full(V, -np.inf, np.float32), V))     # F empty
        for badv in (np.nan, np.inf):
            y = np.zeros(V, np.float32); y[V - 1] = badv
            assert np.isnan(R.reference(y, V))
            y = np.zeros(V + 1, np.float32); y[V] = badv                     # ... but not behind V
            assert abs(R.reference(y, V) - np.log(V)) < 1e-12
    rng = np.random.default_rng(0)
    for _ in range(20):
        x = rng.uniform(-60, 60, 50)
        p = np.exp(x - x.max()); p /= p.sum()
        want = -(p[p > 0] * np.log(p[p > 0])).sum()
        assert abs(R.reference(x, 50) - want) < 1e-12 and 0 <= R.reference(x, 50) <= np.log(50)


def test_merge_rule_equals_direct_evaluation():
    rng = np.random.default_rng(1)
    for trial in range(200):
        n = int(rng.integers(2, 400))
        x = rng.uniform(-60, 60, n)
        x[rng.random(n) < 0.2] = -np.inf
        cuts = np.sort(rng.integers(0, n + 1, int(rng.integers(1, 17))))
        parts = [R.direct(seg) for seg in np.split(x, cuts)]
        if trial % 2:                                                        # merged in two levels, as thread -> slice -> row
            k = len(parts) // 2
            parts = [R.merge(parts[:k]), R.merge(parts[k:])]
        M, S, Z = R.merge(parts)
        m, s, z = R.direct(x)
        if m == -np.inf:
            assert M == -np.inf and S == 0.0
            continue
        assert M == m and abs(S - s) <= 1e-12 * s and abs(Z - z) <= 1e-12 * max(1.0, abs(z))
        assert abs((np.log(S) - Z / S) - R.reference(x, n)) < 1e-10


@pytest.mark.parametrize("V", [V_TINY, V_LARGE])
def test_kernel_model_inside_the_bound_and_planted_faults_outside(V):
    worst = 0.0
    for name, x in R.crafted_rows(V, seed=V):
        ref = R.reference(x, V)
        b = R.bound(x, V)
        got = float(R.kernel_model(x, V))
        err = abs(got - ref)
        worst = max(worst, err / b)
        print(f"V={V} {name}: H={ref:.6f} model err={err:.3e} bound={b:.3e}")
        assert err <= b, (name, got, ref, err, b)
        assert abs(float(R.kernel_model(x, V, fault="pad")) - ref) > 100 * b, name       # +75 in the pad columns takes all mass
        if name in ("slices_at_different_heights", "spread"):
            assert abs(float(R.kernel_model(x, V, fault="noshift")) - ref) > 100 * b, name
    print("worst model |err| / bound", worst)
    assert b < 1e-3                                                                       # the bound is a tolerance, not a licence


def test_kernel_model_special_rows():
    V = V_TINY
    ldv = (V + 3) & ~3
    x = np.full(ldv, 75.0, np.float32); x[:V] = 0.5
    assert abs(float(R.kernel_model(x, V)) - np.log(V)) <= R.bound(x, V)
    x[:V] = -np.inf; x[V - 1] = 3.0
    assert float(R.kernel_model(x, V)) == 0.0
    x[:V] = -np.inf
    assert np.isnan(R.kernel_model(x, V))
    x[:V] = 0.0; x[5] = np.nan
    assert np.isnan(R.kernel_model(x, V))


def test_first_order_term_covers_a_perturbation():
    rng = np.random.default_rng(3)
    for _ in range(50):
        V = 200
        x = rng.uniform(-8, 8, V)
        delta = 10.0 ** rng.uniform(-6, -2)
        y = x + rng.uniform(-delta, delta, V)
        assert abs(R.reference(y, V) - R.reference(x, V)) <= R.first_order(x, V, delta)
