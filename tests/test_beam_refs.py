"""CPU proof that the comparator of tests/beam_refs.py rejects every planted fault of the two-stage beam candidate selection and
accepts the unfaulted float32 model, that no table row is undecidable, that the slice geometry the tables rely on is what they
assume, that the containment claim in the kernels' header comment holds, and that the numpy restatement of resid_grid is exact
for the next-step embedding rows tests/test_gpu_decode_attention.py checks."""
import numpy as np
import pytest

from tests import beam_refs as B
from tests import helpers as Hh

VOCABS = ["tiny", "large"]
N_CANDS = {"tiny": [1, 2, 10, 64], "large": [10, 64]}


def test_geometry_the_tables_rely_on():
    t, l = B.gram("tiny"), B.gram("large")
    assert l.V == 51866 and l.per == 3242 and l.Vpad == 51868 and t.Vpad > t.V
    for G in (t, l):
        assert B.PER_LANE * B.THREADS >= G.per                             # 13 loads cover a slice
        assert (B.NS - 1) * G.per < G.V <= B.NS * G.per                     # 16 slices, none empty
        assert G.slice_of(G.tb - 1) == G.slice_of(G.tb)                     # one slice holds text and timestamp tokens
    assert l.slice_of(l.tb) == 15 and l.bounds(15) == (48630, 51866) and l.bounds(15)[1] - l.bounds(15)[0] == 3236
    assert (B.PER_LANE - 1) * B.THREADS < l.per                              # the 13th load is used, and ragged: 170 of 256 threads
    assert l.per - (B.PER_LANE - 1) * B.THREADS == 170
    assert t.slice_of(t.tb) == 2 and t.per == 111 and t.bounds(15)[1] - t.bounds(15)[0] == 104
    assert t.per <= B.THREADS                                                # tiny: one load per thread, two waves per slice


@pytest.mark.parametrize("which", VOCABS)
def test_no_table_row_is_undecidable(which):
    rows, refs = B.table(which)
    names = [r[0] for r in rows]
    assert len(set(names)) == len(names) and len(rows) > 100
    bad = [(n, r.margin) for n, r in zip(names, refs) if not r.decidable]
    assert not bad, bad
    tie = refs[names.index("case:logsumexp_equal_is_not_greater_tie_to_text")]
    assert tie.margin == 0.0 and tie.ids[:2].tolist() == sorted(tie.ids[:2].tolist()) and tie.ids[0] < B.gram(which).tb
    # what the rows are for: some pad the list, one has no candidate, one holds a NaN, forced and unforced rows both exist
    assert refs[names.index("all_minus_inf")].n == 0 and refs[names.index("nan_above_everything")].nan
    assert refs[names.index("begin_state_allows_51_timestamps")].n == 51 and refs[names.index("five_allowed_tokens")].n <= 5
    G = B.gram(which)
    forced = [r.n > 0 and r.margin > 0 and (r.ids[:r.n] >= G.tb).all() for r in refs]
    assert sum(forced) > 10 and sum(np.isfinite(r.margin) and r.margin < 0 for r in refs) > 10


@pytest.mark.parametrize("which", VOCABS)
def test_clean_model_passes_everywhere(which):
    G = B.gram(which)
    rows, refs = B.table(which)
    worst = 0.0
    for n_cand in N_CANDS[which]:
        for (name, ids, x, mn), r in zip(rows, refs):
            gi, gv = B.kernel_model(G, ids, x, mn, n_cand)
            ok, w, why = B.compare(gi, gv, r, n_cand, "two_stage")
            assert ok, (name, n_cand, why)
            worst = max(worst, w)
    print(f"{which}: clean model, worst |err| / bound = {worst:.3f}")
    assert worst < 1.0


@pytest.mark.parametrize("fault", B.FAULTS)
@pytest.mark.parametrize("which", VOCABS)
def test_every_planted_fault_is_rejected(which, fault):
    G = B.gram(which)
    rows, refs = B.table(which)
    if fault == "load13" and G.per <= (B.PER_LANE - 1) * B.THREADS:
        # no thread of this vocabulary has a 13th element: the fault cannot exist here, and the model must say so
        for (name, ids, x, mn), r in list(zip(rows, refs))[:20]:
            a, b = B.kernel_model(G, ids, x, mn, 10), B.kernel_model(G, ids, x, mn, 10, fault)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        return
    caught = []
    for n_cand in (10, 64):
        for (name, ids, x, mn), r in zip(rows, refs):
            gi, gv = B.kernel_model(G, ids, x, mn, n_cand, fault)
            if not B.compare(gi, gv, r, n_cand, "two_stage")[0]:
                caught.append((name, n_cand))
                break
        if caught:
            break
    print(f"{which}: fault {fault} first rejected on {caught[:1]}")
    assert caught, f"{which}: fault {fault} passes the comparator on every row"


def test_comparator_rejects_a_value_outside_the_bound_and_a_wrong_padding():
    G = B.gram("tiny")
    rows, refs = B.table("tiny")
    i = [r[0] for r in rows].index("five_allowed_tokens")
    name, ids, x, mn = rows[i]
    gi, gv = B.kernel_model(G, ids, x, mn, 10)
    assert B.compare(gi, gv, refs[i], 10, "two_stage")[0] and B.compare(gi, gv, refs[i], 10, "single_block")[0]
    v2 = gv.copy(); v2[0] += np.float32(1e-4)
    assert not B.compare(gi, v2, refs[i], 10, "two_stage")[0]
    v2 = gv.copy(); v2[-1] = np.nan
    assert not B.compare(gi, v2, refs[i], 10, "two_stage")[0]
    i2 = gi.copy(); i2[-1] = 0
    assert not B.compare(i2, gv, refs[i], 10, "two_stage")[0]


@pytest.mark.parametrize("K", [1, 2, 5])
def test_global_top_2k_is_contained_in_the_union_of_the_row_lists(K):
    """The header comment of beam_topk_kernel: the global top 2K over K rows x V of score[r] + processed lp[r], in (value desc,
    flattened index asc) order, equals the top 2K of the union of the per-row top-2K lists.  Tie-heavy rows: few distinct values."""
    G = B.gram("tiny")
    rng = np.random.default_rng(40 + K)
    rows, refs = B.table("tiny")
    names = [r[0] for r in rows]
    pool = [i for i, n in enumerate(names) if n.startswith(("tie_", "all_winners", "text_and_timestamp")) and refs[i].n >= 2 * K]
    for trial in range(6):
        sel = rng.choice(pool, K, replace=False)
        score = np.round(rng.standard_normal(K) * 2) * 0.25 if trial % 2 else np.zeros(K)      # ties across rows as well
        # full float64 processed log-probabilities of the rows
        full = np.full((K, G.V), -np.inf)
        lists = []
        for k, i in enumerate(sel):
            name, ids, x, mn = rows[i]
            x64 = x.astype(np.float64)
            lp = x64 - (x64.max() + np.log(np.exp(x64 - x64.max()).sum()))
            quant = np.round(lp * 4) / 4                                                             # more ties still
            out = B.OL.process(G.spec(mn), ids[None], x[None], B.N_PROMPT, B.N_PROMPT)[0]
            full[k] = np.where(np.isfinite(out), quant, -np.inf) + score[k]
            keep = np.flatnonzero(np.isfinite(full[k]))
            order = keep[np.lexsort((keep, -full[k][keep]))][:2 * K]
            lists += [(full[k][v], k * G.V + v) for v in order]
        flat = full.reshape(-1)
        keep = np.flatnonzero(np.isfinite(flat))
        want = keep[np.lexsort((keep, -flat[keep]))][:2 * K].tolist()
        got = [i for _, i in sorted(lists, key=lambda p: (-p[0], p[1]))][:2 * K]
        assert got == want, (K, trial)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_resid_grid_restatement_is_exact_for_the_embedding_rows(dt):
    """x = resid_grid(embed16[tok] + pos_embed[t]) as beam_commit_kernel stores it: the f32 sum is rounded once, v * 4096 and
    * 2^-12 are exact in f32, so the numpy restatement in float32 equals the same rule evaluated in float64 on the f32 sum."""
    import torch
    g, v, W, spec = Hh.tiny_setup()
    e = torch.from_numpy(np.ascontiguousarray(W["model.decoder.embed_tokens.weight"], np.float32))
    e = e.to(torch.bfloat16 if dt == "bf16" else torch.float16).float().numpy()
    pe = np.asarray(W["model.decoder.embed_positions.weight"], np.float32)
    rng = np.random.default_rng(3)
    tok = rng.integers(0, v.size, 64)
    t = rng.integers(0, spec.max_target_positions, 64)
    s = (e[tok] + pe[t]).astype(np.float32)                       # one f32 addition, as Act<T>::ld(e) + pe
    got = B.resid_grid(s)
    want = np.rint(s.astype(np.float64) * 4096.0) / 4096.0
    assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want)
    assert np.abs(s).max() * 4096 < 2 ** 24                       # rint(v * 4096) is an integer f32 holds exactly
    assert np.any(got != s)                                        # ... and the grid does move these values
    # half-way cases go to even, as rintf does
    assert B.resid_grid(np.float32([0.5 / 4096, 1.5 / 4096, 2.5 / 4096, -0.5 / 4096])).tolist() == [0.0, 2 / 4096, 2 / 4096, -0.0]
