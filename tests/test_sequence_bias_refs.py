"""tests/sequence_bias_refs.py against the installed transformers SequenceBiasLogitsProcessor itself: ``processor(ids, zeros)``
equals ``dense_bias`` bit for bit, the argument checks agree, and each planted fault is rejected by the same comparison."""
import numpy as np
import pytest

from tests import sequence_bias_refs as S

torch = pytest.importorskip("torch")
lp = pytest.importorskip("transformers.generation.logits_process")
Proc = lp.SequenceBiasLogitsProcessor

V = 97


def _tf(ids, table_arg):
    """The processor's own bias: its output on all-zero scores."""
    ids = np.asarray(ids, np.int64)
    out = Proc(table_arg)(torch.from_numpy(ids), torch.zeros(ids.shape[0], V, dtype=torch.float32))
    return out.numpy().astype(np.float32)


def _crafted():
    """(name, ids [nb][t], transformers argument)"""
    P = [50, 51, 52]                                                # a three-token prompt
    out = []
    out.append(("single", [P + [7, 8]], [[[9], 2.5]]))
    out.append(("L_equals_cur_len_applies", [[5, 6, 7]], [[[5, 6, 7, 8], 1.0], [[6, 7, 8], 3.0]]))   # L = 4 > 3 skipped, L = 3 applies
    out.append(("L_is_cur_len_plus_one_skipped", [[6, 7]], [[[6, 7, 8], 3.0]]))
    out.append(("two_applying_same_last_token_order_matters", [P + [3, 4]], [[[4, 9], 1e8], [[3, 4, 9], -1e8], [[9], 1.0]]))
    out.append(("same_last_token_other_order", [P + [3, 4]], [[[9], 1.0], [[3, 4, 9], -1e8], [[4, 9], 1e8]]))
    out.append(("prefix_reaches_into_prompt", [P + [3]], [[[51, 52, 3, 11], 4.0], [[52, 3, 12], -2.0], [[50, 52, 3, 13], 9.0]]))
    out.append(("rows_differ", [P + [3, 4], P + [4, 4], P + [3, 5], P + [5, 3]], [[[3, 4, 9], 1.5], [[4, 9], 0.25], [[5, 9], -7.0], [[9], 0.125]]))
    out.append(("dict_form", [P + [3, 4]], {(4, 9): 2.0, (9,): 1.0, (0, 4, 9): 5.0, (3, 4, 9): 0.5}))
    out.append(("duplicates_in_list_form_last_wins", [P + [3, 4]], [[[4, 9], 1e8], [[9], 1.0], [[4, 9], -3.0], [[3, 4, 9], 1e8], [[9], 2.0]]))
    out.append(("length_16", [list(range(20, 40))], [[list(range(25, 40)) + [1], 6.0], [list(range(24, 39)) + [1], 7.0]]))
    return out


def _random(rng, n):
    out = []
    for i in range(n):
        nb, t = int(rng.integers(1, 6)), int(rng.integers(1, 12))
        ids = rng.integers(1, 8, size=(nb, t))                      # a small alphabet: prefixes do match
        table = []
        for _ in range(int(rng.integers(1, 12))):
            L = int(rng.integers(1, 6))
            if rng.random() < 0.5 and L - 1 <= t and L > 1:         # lifted from a row, so that it applies there
                b = int(rng.integers(0, nb))
                seq = ids[b, t - (L - 1):].tolist() + [int(rng.integers(1, V))]
            else:
                seq = rng.integers(1, 8, size=L - 1).tolist() + [int(rng.integers(1, 12))]
            table.append([[int(x) for x in seq], float(np.float32(rng.standard_normal() * 10.0 ** int(rng.integers(-2, 9))))])
        out.append((f"random{i}", ids.tolist(), table))
    return out


CASES = _crafted() + _random(np.random.default_rng(0), 60)


@pytest.mark.parametrize("name, ids, arg", CASES, ids=[c[0] for c in CASES])
def test_dense_bias_is_the_processors(name, ids, arg):
    ids = np.asarray(ids, np.int64)
    want = _tf(ids, arg)
    got = S.dense_bias(ids, ids.shape[1], S.validate(arg, V), V)
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), (name, np.flatnonzero(got != want))
    lg = np.random.default_rng(1).standard_normal((len(ids), V)).astype(np.float32)
    full = Proc(arg)(torch.from_numpy(ids), torch.from_numpy(lg)).numpy()
    assert S.biased(lg, ids, ids.shape[1], S.validate(arg, V)).tobytes() == full.tobytes()


def test_what_the_crafted_cases_are_for():
    c = {n: (np.asarray(i), S.validate(a, V)) for n, i, a in _crafted()}
    d = lambda n: S.dense_bias(c[n][0], c[n][0].shape[1], c[n][1], V)
    assert d("L_equals_cur_len_applies")[0, 8] == 3.0
    assert not d("L_is_cur_len_plus_one_skipped").any()
    assert d("two_applying_same_last_token_order_matters")[0, 9] == 0.0        # (1 + 1e8) - 1e8 in float32
    assert d("same_last_token_other_order")[0, 9] == 0.0 and c["same_last_token_other_order"][1][0] == ((9,), 1.0)
    pr = d("prefix_reaches_into_prompt")[0]
    assert pr[11] == 4.0 and pr[12] == -2.0 and pr[13] == 0.0
    r = d("rows_differ")[:, 9]
    assert r.tolist() == [1.5 + 0.25 + 0.125, 0.25 + 0.125, -7.0 + 0.125, 0.125]
    dup = c["duplicates_in_list_form_last_wins"][1]
    assert dup == [((4, 9), -3.0), ((9,), 2.0), ((3, 4, 9), 1e8)]
    assert d("length_16")[0, 1] == 6.0


@pytest.mark.parametrize("fault", S.FAULTS)
def test_planted_faults_are_rejected(fault):
    bad = 0
    for name, ids, arg in CASES:
        ids = np.asarray(ids, np.int64)
        if S.dense_bias(ids, ids.shape[1], S.validate(arg, V), V, fault=fault).tobytes() != _tf(ids, arg).tobytes():
            bad += 1
    assert bad > 0, fault


MALFORMED = [
    [], {}, None, "x", 3,
    {(1, 2): 1.0, 3: 2.0}, {(): 1.0}, {(1, -2): 1.0}, {(1, 2.0): 1.0}, {(1, 2): 1}, {(1,): "a"},
    [[[1, 2], 1]], [[[1, 0], 1.0]], [[[1, -1], 1.0]], [[(1, 2), 1.0]], [[[1.5], 1.0]], [[1, 1.0]],
]


@pytest.mark.parametrize("arg", MALFORMED, ids=[repr(a) for a in MALFORMED])
def test_malformed_arguments_are_refused_like_transformers(arg):
    with pytest.raises(Exception):
        Proc(arg)                                                    # transformers refuses it ...
    with pytest.raises(ValueError):
        S.validate(arg)                                              # ... and so does the restatement
    from crisperwhisper_amd import generation
    if arg is not None:
        with pytest.raises(ValueError):
            generation.check_sequence_bias(arg, V)


@pytest.mark.parametrize("arg", [[[[5], 1.0]], {(0, 5): 1.0}, [[[1, 2], 1.0], [[1, 2], 2.0]]])
def test_well_formed_arguments_pass_both(arg):
    from crisperwhisper_amd import generation
    Proc(arg)
    assert S.validate(arg, V) == generation.check_sequence_bias(arg, V)


@pytest.mark.parametrize("arg", [[[[V], 1.0]], [[[1], float("inf")]], [[[1], float("nan")]], [[[1] * 17, 1.0]],
                                 [[[i + 1, 1], 1.0] for i in range(257)], [[[], 1.0]]])
def test_what_the_engine_adds_to_the_refusals(arg):
    from crisperwhisper_amd import generation
    with pytest.raises(ValueError):
        S.validate(arg, V)
    with pytest.raises(ValueError):
        generation.check_sequence_bias(arg, V + 200 if len(arg) > 1 else V)
