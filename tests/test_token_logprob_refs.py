"""The comparator of tests/token_logprob_refs.py accepts the float32 model of the sampler's log-probability reduction and rejects
every planted fault on the crafted rows: pad columns included in the sum, masked tokens left out (the processed denominator of
lp_sum), slice maxima merged without rescaling, a one-position shift, the arg-max's value reported for a forced token.
Host-only: no GPU."""
import numpy as np
import pytest

from tests import token_logprob_refs as R

VOCABS = [1001, 51866]          # neither is a multiple of 4: there are pad columns


@pytest.fixture(scope="module", params=VOCABS)
def rows(request):
    V = request.param
    return V, R.crafted_rows(V, seed=V)


def test_the_model_without_a_fault_is_inside_the_bound(rows):
    V, cs = rows
    for name, x, dead, tok, am in cs:
        ok, err, bd = R.compare(R.kernel_model(x, tok, V, dead), x, tok, V)
        print(V, name, err, bd)
        assert ok, (name, err, bd)
        assert bd < 1e-4, (name, bd)               # the bound stays a rounding bound: far below any fault planted here


@pytest.mark.parametrize("fault", ["pad", "masked", "norescale"])
def test_a_faulty_reduction_is_rejected(rows, fault):
    V, cs = rows
    for name, x, dead, tok, am in cs:
        got = R.kernel_model(x, tok, V, dead, fault=fault)
        ok, err, bd = R.compare(got, x, tok, V)
        print(V, fault, name, err, bd)
        assert not ok, (fault, name, err, bd)


def test_a_one_position_shift_is_rejected(rows):
    V, cs = rows
    vals = [R.kernel_model(x, tok, V, dead) for name, x, dead, tok, am in cs]
    for k, (name, x, dead, tok, am) in enumerate(cs):
        shifted = vals[(k + 1) % len(vals)]         # the value of the neighbouring step
        ok, err, bd = R.compare(shifted, x, tok, V)
        assert not ok, (name, err, bd)


def test_the_argmax_value_for_a_forced_token_is_rejected(rows):
    V, cs = rows
    hit = 0
    for name, x, dead, tok, am in cs:
        if tok == am:
            continue
        hit += 1
        ok, err, bd = R.compare(R.kernel_model(x, am, V, dead), x, tok, V)
        assert not ok, (name, err, bd)
    assert hit >= 3


def test_degenerate_rows():
    V = 1001
    x = np.full(1004, -np.inf, np.float32)
    assert R.compare(np.float32(np.nan), x, 5, V)[0] and not R.compare(np.float32(0.0), x, 5, V)[0]
    x[:V] = 0.0; x[7] = -np.inf
    assert R.compare(np.float32(-np.inf), x, 7, V)[0] and not R.compare(np.float32(-1.0), x, 7, V)[0]
    assert R.compare(R.kernel_model(x, 3, V), x, 3, V)[0]
    assert R.n_iter(51866) == 4 and R.n_iter(1001) == 1
