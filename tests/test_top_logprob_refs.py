"""The float64 reference of the alternatives (tests/top_logprob_refs.py) accepts a faithful float32 model of the kernels'
two-stage selection and rejects every planted fault on the crafted rows -- on the CPU, so the GPU tests' comparator is known to
bite before it is pointed at the kernels."""
import numpy as np
import pytest

from tests import token_logprob_refs as R
from tests import top_logprob_refs as T

VOCABS = [1769, 51866]          # one float4 group per thread with pad columns; four groups per thread, last slice short


def test_reference_orders_by_value_then_id_and_pads():
    x = np.array([1.0, 5.0, -np.inf, 5.0, np.nan, 2.0, 99.0, 99.0], np.float32)      # V = 6: the two 99 are pad columns
    ids, lps = T.reference_topk(x, 6, 5)
    assert ids.tolist() == [1, 3, 5, 0, -1]
    assert np.isnan(lps).all()                                  # the NaN logit poisons the normaliser, as for the token's own value
    x[4] = -3.0
    ids, lps = T.reference_topk(x, 6, 5)
    assert ids.tolist() == [1, 3, 5, 0, 4]
    lse = np.log(np.exp(np.array([1.0, 5.0, 5.0, -3.0, 2.0], np.float64)).sum())
    assert np.allclose(lps, np.array([5.0, 5.0, 2.0, 1.0, -3.0]) - lse, rtol=0, atol=1e-12)
    ids, lps = T.reference_topk(np.full(8, -np.inf, np.float32), 6, 3)
    assert ids.tolist() == [-1, -1, -1] and np.isnan(lps).all()


@pytest.mark.parametrize("k", [1, 5, 8])
@pytest.mark.parametrize("V", VOCABS)
def test_the_faithful_model_passes_on_every_crafted_row(V, k):
    for name, x, dead in T.crafted_rows(V, k):
        ids, lps = T.kernel_model_topk(x, V, k, dead)
        ok, worst, why = T.compare_topk(ids, lps, x, V, k)
        assert ok, (name, why)
        assert worst <= 1.0
    rng = np.random.default_rng(V + k)
    ldv = T.geometry(V)[0]
    x = rng.uniform(-60, 60, ldv).astype(np.float32)
    ids, lps = T.kernel_model_topk(x, V, k, rng.random(V) < 0.3)
    assert T.compare_topk(ids, lps, x, V, k)[0]


@pytest.mark.parametrize("fault", T.FAULTS)
@pytest.mark.parametrize("V", VOCABS)
def test_every_planted_fault_is_rejected(V, fault):
    k = 5
    rejected = []
    for name, x, dead in T.crafted_rows(V, k):
        ids, lps = T.kernel_model_topk(x, V, k, dead, fault=fault)
        ok, _, why = T.compare_topk(ids, lps, x, V, k)
        if not ok:
            rejected.append(name)
    print(V, fault, "rejected on", rejected)
    assert rejected, f"fault {fault!r} passes the comparator on every crafted row"
    want = {"pad": "winners_in_the_last_float4", "tie_high": "tie_across_slice_boundary",
            "masked": "all_winners_in_one_slice_half_masked", "repeat": "slices_with_0_1_and_k-1_finite",
            "best_only": "all_winners_in_one_slice_half_masked", "processed_sum": "all_winners_in_one_slice_half_masked"}[fault]
    assert want in rejected


def test_the_written_token_among_the_alternatives_has_the_same_value():
    """The model's value of an alternative is the model's token log-probability of that id: one arithmetic."""
    V, k = 1769, 8
    for name, x, dead in T.crafted_rows(V, k):
        ids, lps = T.kernel_model_topk(x, V, k, dead)
        if np.isnan(x[:V]).any():
            continue
        for i, lp in zip(ids, lps):
            if i >= 0:
                assert np.float32(lp).tobytes() == np.float32(R.kernel_model(x, int(i), V, dead)).tobytes()
