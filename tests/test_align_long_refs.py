"""Self-checks of tests/align_long_refs.py against brute force: every S[n] recomputed on its own with math.fsum (exactly rounded),
the arg-max confirmed by enumeration.  Where two candidates lie within 1e-9 of each other only the documented tie rule (the
lowest n of an exact tie) is asserted; the restatement's own sequential float64 sum decides between near-ties."""
import math

import numpy as np
import pytest

from tests import align_long_refs as R


def _case(rng, N, kind):
    lp = (-rng.exponential(2.0, N + 1)).astype(np.float32)
    st = (-rng.exponential(6.0, N + 1)).astype(np.float32)
    if kind == "inf":
        st[rng.integers(0, N + 1, max(1, N // 3))] = -np.inf
    mask = rng.random(N + 1) < 0.4
    mask[rng.integers(0, N + 1)] = True
    return lp, st, mask


@pytest.mark.parametrize("N", [0, 1, 2, 17, 64, 444])
@pytest.mark.parametrize("kind", ["plain", "inf"])
def test_cut_against_enumeration(N, kind):
    rng = np.random.default_rng(1000 + N)
    for _ in range(20):
        lp, st, mask = _case(rng, N, kind)
        S = [math.fsum([float(x) for x in lp[:n]]) + float(st[n]) for n in range(N + 1)]
        got, score = R.cut(lp, st, mask, False)
        assert mask[got]
        allowed = [n for n in range(N + 1) if mask[n]]
        top = max(S[n] for n in allowed)
        assert S[got] >= top - 1e-9 or (top == -math.inf and S[got] == -math.inf)
        near = [n for n in allowed if S[n] >= top - 1e-9 or S[n] == top]
        if len(near) == 1:
            assert got == near[0]
        if np.isfinite(S[got]):
            assert abs(float(score) - S[got]) <= abs(S[got]) * 2.0 ** -23 + 1e-30
        else:
            assert score == np.float32(-np.inf)
        forced, fscore = R.cut(lp, st, np.zeros(N + 1, bool), True)
        assert forced == N and (fscore == np.float32(R.prefix_scores(lp, st)[N]))


def test_exact_tie_takes_the_lowest_n():
    # S[1] == S[3] exactly: lp sums to 0 between them and the stop entries are equal
    lp = np.array([-1.0, -0.5, 0.0, -2.0, -1.0], np.float32)
    st = np.array([-9.0, -3.0, -7.0, -3.5, -8.0], np.float32)
    st[3] = np.float32(-3.0 + 0.5)                      # S[1] = -1 - 3 = -4; S[3] = -1.5 - 2.5 = -4
    S = R.prefix_scores(lp, st)
    assert S[1] == S[3] == -4.0
    assert R.cut(lp, st, [1, 1, 1, 1, 1], False)[0] == 1
    assert R.cut(lp, st, [1, 0, 1, 1, 1], False)[0] == 3
    assert R.cut(lp, st, [0, 0, 0, 0, 0], True)[0] == 4
    with pytest.raises(ValueError):
        R.cut(lp, st, [0, 0, 0, 0, 0], False)
    allinf = np.full(5, -np.inf, np.float32)
    assert R.cut(lp, allinf, [0, 1, 0, 1, 0], False)[0] == 1          # a tie at -inf is a tie


def test_stop_logprob_against_enumeration():
    rng = np.random.default_rng(5)
    for V, eos, tb in ((48, 3, 45), (250, 17, 250), (250, 200, 240)):
        l = rng.standard_normal((6, V)) * 8
        l[1, tb - 1 if tb < V else eos] = 60.0
        l[2] -= 0.0
        l[2, :] = np.where(R.stop_set(V, eos, tb), l[2] - 150.0, l[2])   # S far under the row maximum
        got = R.stop_logprob(l, eos, tb)
        for m in range(6):
            p = [math.exp(x - l[m].max()) for x in l[m]]
            ps = [p[n] for n in range(V) if n == eos or n >= tb]
            tot = math.fsum(p)
            if math.fsum(ps) > 0:
                want = math.log(math.fsum(ps)) - math.log(tot)
                assert abs(got[m] - want) <= 1e-9 * (1 + abs(want))
            else:                                        # underflows against the row maximum: the own-maximum form does not
                assert np.isfinite(got[m]) and got[m] < -100
        assert np.all(got <= 1e-12)
        assert R.stop_logprob(l[0], eos, tb) == got[0]
