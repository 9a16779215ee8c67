"""The comparator of the score top_logprobs GPU tests (tests/score_top_refs.py) rejects every planted fault of the numpy model of
the head's split / list / merge selection, and passes the clean model in both orders of service."""
import numpy as np
import pytest

from tests import score_top_refs as R

V, TPS = 250, 4                                   # 15 x 16 + 10 columns: four splits of one tile group, a ragged last tile


def _case():
    """f32 logits [4][256]; columns 250 .. 255 are the padding columns, copies of column V - 1 as in the packed image."""
    rng = np.random.default_rng(5)
    z = (rng.standard_normal((4, 256)) - 6.0).astype(np.float32)          # all negative: a stale (0.0, id 0) pair would win
    z[0, V - 1] = 3.0                             # row 0: the column next to the padding is the best
    z[0, [70, 130, 200]] = 2.5                    # ... and three identical values in three splits: ids ascending
    # row 1: seven of the 8 best in one lane's and its neighbour's columns of the first tile group; rank 7 is an exact tie in
    # the second tile group that lane order meets high id first
    z[1, [3, 19, 35, 51, 5, 21, 37]] = [9, 8, 7, 6, 5, 4, 3]
    z[1, 112] = 2.0                               # lane 0's column of tile 7 ...
    z[1, 65] = 2.0                                # ... ties with lane 1's column of tile 4: id 65 is rank 7, id 112 is out
    z[2] = -np.arange(256, dtype=np.float32)      # strictly descending in the id: no insertion after the fill
    z[3] = np.arange(256, dtype=np.float32) - 300  # strictly ascending: every column inserts
    z[3, 17] = -np.inf
    z[:, V:] = z[:, V - 1:V]
    return z


@pytest.mark.parametrize("order", ["tile", "lane"])
@pytest.mark.parametrize("tps", [TPS, 8])
@pytest.mark.parametrize("k", [1, 3, 8])
def test_clean_model_passes(order, k, tps):
    z = _case()
    ids, lp = R.model_topk(z, V, k, tps, order=order)
    problems, worst = R.check_topk(ids, lp, z, V, k, V / 16, R.HEAD_C)
    assert not problems, problems
    assert worst <= 1.0
    ref, _, _ = R.reference_topk(z, V, 8)
    assert ref[0, :4].tolist() == [V - 1, 70, 130, 200] and ref[1, 7] == 65 and 112 not in ref[1]
    assert ref[2].tolist() == list(range(8)) and ref[3].tolist() == list(range(V - 1, V - 9, -1))


@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_fault_is_rejected(fault):
    z = _case()
    order = "lane" if fault == "value_only" else "tile"       # (in tile order a row meets its ids ascending: value alone suffices)
    # value_only needs a full list before the tie arrives: two tile groups per split
    ids, lp = R.model_topk(z, V, 8, 8 if fault == "value_only" else TPS, fault=fault, order=order)
    problems, _ = R.check_topk(ids, lp, z, V, 8, V / 16, R.HEAD_C)
    assert problems, fault


def test_comparator_rejects_value_and_padding_errors():
    z = _case()
    ids, lp = R.model_topk(z, V, 3, TPS)
    bad = lp.copy(); bad[1, 2] += np.float32(1e-3)
    assert R.check_topk(ids, bad, z, V, 3, V / 16, R.HEAD_C)[0]
    bad = lp.copy(); bad[1, 5] = 0.0                          # rank >= k must stay NaN
    assert R.check_topk(ids, bad, z, V, 3, V / 16, R.HEAD_C)[0]
    bad = ids.copy(); bad[0, 0], bad[0, 1] = ids[0, 1], ids[0, 0]
    assert R.check_topk(bad, lp, z, V, 3, V / 16, R.HEAD_C)[0]


def test_reference_edge_rows():
    z = np.full((3, 8), -np.inf, np.float32)
    z[1, [2, 5]] = [1.0, np.nan]
    z[2, :5] = [0.5, 0.5, np.nan, -np.inf, 0.25]
    ids, lp, lse = R.reference_topk(z, 5, 8)
    assert ids[0].tolist() == [-1] * 8 and np.isnan(lp[0]).all()
    assert ids[1].tolist() == [2] + [-1] * 7                  # column 5 is >= V
    assert ids[2].tolist() == [0, 1, 4] + [-1] * 5 and np.isnan(lse[2])
