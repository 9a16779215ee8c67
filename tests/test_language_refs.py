"""The comparator of tests/language_refs.py on the float32 model of the language-identification kernel: it accepts the clean
model on every crafted and random row and rejects every planted fault -- so a GPU run that passes it has none of them."""
import numpy as np
import pytest

from tests import language_refs as R

V_SMALL, V_LARGE = 1111, 51866


def _table(V, n, seed):
    """n distinct ids in one contiguous range of the vocabulary (as the language tokens are), shuffled: table order != id order."""
    rng = np.random.default_rng(seed)
    lo = V // 2
    ids = lo + rng.permutation(n)
    if n > 1 and not np.any(np.diff(ids) < 0):
        ids = ids[::-1]
    return ids.astype(np.int32)


def _ns_tok(V):
    return V - 40


@pytest.mark.parametrize("V,n", [(V_SMALL, 1), (V_SMALL, 2), (V_SMALL, 4), (V_SMALL, 99), (V_SMALL, 128), (V_LARGE, 100)])
def test_comparator_accepts_the_clean_model(V, n):
    ids, tok = _table(V, n, 3 + n), _ns_tok(V)
    rows = [x for _, x in R.crafted_rows(V, ids, tok)]
    ldv = len(rows[0])
    for r in R.random_rows(V, 4, 17 + n):
        x = np.full(ldv, 75.0, np.float32); x[:V] = r
        rows.append(x)
    out = [R.kernel_model(x, ids, V, tok) for x in rows]
    R.check_rows([o[0] for o in out], [o[1] for o in out], [o[2] for o in out], rows, ids, V, tok, what=f"model V={V} n={n}")


def test_the_definition_on_hand_computed_rows():
    V, ids = 13, np.array([7, 3, 5], np.int32)
    x = np.zeros(16, np.float32); x[V:] = 75.0
    x[[7, 3, 5]] = np.log([1.0, 2.0, 5.0]).astype(np.float32)
    best, prob, ns = R.reference(x, ids, V, 0)
    assert best == 5 and np.allclose(prob, [0.125, 0.25, 0.625], atol=1e-7)           # table order, candidates only
    assert abs(ns - 1.0 / (10 + 8)) < 1e-7                                            # ten columns at 0, 1 + 2 + 5; no pad column
    x[3] = x[5]
    assert R.reference(x, ids, V, -1)[0] == 3                                         # lowest id on an exact tie
    x[[7, 3, 5]] = [-np.inf, np.nan, -np.inf]
    best, prob, _ = R.reference(x, ids, V, -1)
    assert best == 3 and np.isnan(prob).all()
    x[7] = 0.5
    best, prob, _ = R.reference(x, ids, V, -1)
    assert best == 7 and prob.tolist() == [1.0, 0.0, 0.0]                             # a NaN / -inf candidate: exactly 0


@pytest.mark.parametrize("V", [V_SMALL, V_LARGE])
@pytest.mark.parametrize("fault", R.FAULTS)
def test_comparator_rejects_every_fault(fault, V):
    n = 100
    ids, tok = _table(V, n, 11), _ns_tok(V)
    landed = []
    for name, x in R.crafted_rows(V, ids, tok):
        best, prob, ns = R.kernel_model(x, ids, V, tok, fault=fault)
        ok, worst, why = R.compare(best, prob, ns, x, ids, V, tok)
        if not ok:
            landed.append((name, worst, any("best" in w or "must be" in w for w in why)))
    print(fault, V, landed)
    assert landed, f"fault {fault!r} passes the comparator on every crafted row"
    # far outside: an inexact value misses its bound by orders of magnitude, or the exact part -- best, 0, NaN -- is wrong
    assert any(w > 100 or exact for _, w, exact in landed)


def test_bounds_are_first_order_small():
    V = V_LARGE
    ids, tok = _table(V, 100, 5), _ns_tok(V)
    x = np.full((V + 3) & ~3, 75.0, np.float32); x[:V] = R.random_rows(V, 1, 9)[0]
    _, prob, ns = R.reference(x, ids, V, tok)
    assert np.all(R.prob_bound(x, ids) <= prob * 1e-4 + 2 * R.TINY)
    assert R.ns_bound(x, V, tok) <= ns * 1e-4 + 2 * R.TINY
    assert R.n_iter(V) == 51
