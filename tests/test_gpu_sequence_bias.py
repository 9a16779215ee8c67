"""sequence_bias on the device (cw_set_sequence_bias; sample_partial_kernel<TOPK, true> / sample_kernel<T, TOPK, true> in
csrc/elementwise.hip).

Differential, without a tolerance: the sampler under a table on logits X against the same sampler without a table on
fl32(X + dense_bias) (tests/sequence_bias_refs.py, held to transformers' processor bit for bit on the CPU) -- the greedy choice,
the sampled choice under the same seed and streams, the bits of the processed-score log-probability term; the raw outputs (the
token log-probability and the top_logprobs of a pinned token) against the table-free run on X; the greedy choice also against the
float64 processors of tests/sampling_ref.py.  Then real decodes of the tiny model (graph and non-graph path, native and host seek
loop, average log-probability in float64, off / on / off), temperature fallback, transformers' own output under six tables
(tests/golden/gen_golden_sequence_bias.py) and the pipeline."""
import numpy as np
import pytest

import crisperwhisper_amd as cw
from crisperwhisper_amd import audio, collate, generation, synthetic as syn
from crisperwhisper_amd.engine import Engine
from crisperwhisper_amd.generation import stream_id
from tests import helpers as Hh
from tests import sampler_cases as SC
from tests import sampling_ref as R
from tests import sequence_bias_refs as S
from tests.top_logprob_refs import GOLD_GAP, geometry
from tests.test_gpu_token_logprobs import _clips, _prompt

pytestmark = pytest.mark.gpu

K = 5
GOLD = Hh.gold_json("sequence_bias_golden.json")
# The timestamp rule compares log(sum over timestamps of exp(s - m)) with (best text - m).  The f32 side sums at most 1501 terms
# of relative error 2^-22 each (expf within 2 ulp) and takes one logf: the relative error of the sum is below 1505 * 2^-24 = 9e-5
# and so is the absolute error of its logarithm; the subtraction of two scores below 128 adds 2^-24 * 256.  A float64 margin
# below 1e-4 + 1.6e-5 says nothing about which side the f32 rule lands on.
RULE_MARGIN = 1.2e-4


@pytest.fixture(scope="module")
def tiny():
    return Hh.tiny_setup()


@pytest.fixture(scope="module")
def engines(tiny):
    g, v, W, spec = tiny
    out = {}
    for dt in ("f32", "bf16"):
        e = Engine(spec, dtype=dt, max_batch=8)
        e.load_state_dict(W)
        out[dt] = e
    yield out
    for e in out.values():
        e.close()


@pytest.fixture(scope="module")
def large():
    """The sampler at the vocabulary of large-v3 (51 866 columns, four loads per thread, last slice short), one layer, no weights."""
    g, v = syn.large_v3_geometry()
    g.enc_layers = g.dec_layers = 1
    spec = syn.model_spec(g, v, n_align=1)
    spec.alignment_heads = [[0, 0]]
    eng = Engine(spec, dtype="bf16", max_batch=8)
    yield g, v, spec, eng
    eng.close()


def _greedy_ref(spec, xb, ids, mn):
    """(float64 arg-max of the processed scores, whether the timestamp rule is too close to call in f32)."""
    s, _ = R.processed_scores(spec, xb, list(ids), 3, mn)
    tb = spec.timestamp_begin
    no_ts = np.asarray(xb, np.float64).copy()
    no_ts[tb:] = -np.inf                                               # no timestamp mass: the rule cannot fire, the text survives
    text = R.processed_scores(spec, no_ts, list(ids), 3, mn)[0][:tb]
    close = False
    m = max(s[tb:].max(), text.max())
    if np.isfinite(text.max()) and np.isfinite(s[tb:].max()):
        with np.errstate(divide="ignore"):
            close = abs(np.log(np.exp(s[tb:] - m).sum()) - (text.max() - m)) < RULE_MARGIN
    return (int(np.argmax(s)) if np.isfinite(s.max()) else 0), close


def _differential(eng, spec, lg, ids, table, mn=0, seed=7, what=""):
    """Every assertion of the differential on one launch.  Returns the greedy choices under the table."""
    lg = np.ascontiguousarray(lg, np.float32)
    ids = np.ascontiguousarray(ids, np.int32)
    nb, t = ids.shape
    V = spec.vocab_size
    xb = S.biased(lg, ids, t, table)
    streams = [stream_id(b, 3 * b, 1) for b in range(nb)]
    out = None
    for temp in (0.0, 0.7):
        st = streams if temp > 0 else None
        a = eng.test_sample_biased(lg, ids, 3, K, table, temp, seed, st, min_new_tokens=mn)
        b = eng.test_sample_biased(xb, ids, 3, K, None, temp, seed, st, min_new_tokens=mn)
        c = eng.test_sample_top_logprobs(xb, ids, 3, K, temp, seed, st, min_new_tokens=mn)
        assert a[0].tolist() == b[0].tolist() == c[0].tolist(), (what, temp, a[0].tolist(), b[0].tolist())
        assert a[4].tobytes() == b[4].tobytes(), (what, temp, a[4], b[4])                 # the processed-score term, bit for bit
        if temp == 0.0:
            out = a[0].copy()
            n_close = 0
            for r in range(nb):
                want, close = _greedy_ref(spec, xb[r], ids[r], mn)
                n_close += close
                assert close or int(a[0][r]) == want, (what, r, int(a[0][r]), want)
            assert n_close <= max(1, nb // 4), (what, n_close)
    # raw outputs: the token pinned, the table must not move tok_lp nor the alternatives
    forced = np.array([(int(out[r]) + 1 + 17 * r) % V for r in range(nb)], np.int32)
    for temp in (0.0, 0.7):
        st = streams if temp > 0 else None
        a = eng.test_sample_biased(lg, ids, 3, K, table, temp, seed, st, forced=forced, min_new_tokens=mn)
        c = eng.test_sample_top_logprobs(lg, ids, 3, K, temp, seed, st, forced=forced, min_new_tokens=mn)
        assert a[1].tobytes() == c[1].tobytes() and a[2].tobytes() == c[2].tobytes() and a[3].tobytes() == c[3].tobytes(), (what, temp)
        d = eng.test_sample_biased(xb, ids, 3, K, None, temp, seed, st, forced=forced, min_new_tokens=mn)
        assert a[0].tolist() == d[0].tolist() and a[4].tobytes() == d[4].tobytes(), (what, temp)   # forced: the un-forced choice still moves
    return out


def _rows(v, spec, V, nb, seed, t_gen=6):
    """nb rows sharing a length, histories over a small alphabet in a legal grammar state (ts, text ...), random logits."""
    rng = np.random.default_rng(seed)
    tb = spec.timestamp_begin
    alpha = [300, 301, 302] if V > 2000 else [ord("a"), ord("b"), ord("c")]
    ids = np.zeros((nb, 3 + t_gen), np.int32)
    for b in range(nb):
        ids[b] = [v.sot, v.lang_id("en"), v.transcribe, tb + 2] + [alpha[int(x)] for x in rng.integers(0, 3, t_gen - 1)]
    lg = (rng.standard_normal((nb, V)) * 3).astype(np.float32)
    return ids, lg


def _tables(v, spec, V, ids):
    """name -> table for a launch with histories ``ids``: the places where the kernel can go wrong."""
    nb, t = ids.shape
    _, per = geometry(V)
    tb, eos = spec.timestamp_begin, spec.eos_token_id
    X = 310 if V > 2000 else ord("x")                                  # unsuppressed text tokens
    Y = 311 if V > 2000 else ord("y")
    out = {}
    out["slice_edges"] = [((0,), 4.0), ((per - 1,), 6.0), ((15 * per,), -3.0), ((V - 1,), 60.0), ((per,), 5.5), ((15 * per - 1,), 7.25)]
    n1 = min(256, per)
    one = [((3 * per + i,), float(0.5 + i % 7)) for i in range(n1)]    # 256 entries whose last token lies in slice 3
    for i in range(256 - n1):                                          # a slice narrower than 256 columns: two-token entries fill up,
        pre = int(ids[0, -1]) if i < per else int(v.sot)               # half of them applying to row 0
        one.append(((pre, 3 * per + i % per), float(-2.0 - i % 5)))
    out["all_256_in_one_slice"] = one
    last, prev = int(ids[0, -1]), int(ids[0, -2])
    out["order_dependent_sum"] = [((last, X), 1e8), ((prev, last, X), -1e8), ((X,), 1.0),
                                  ((Y,), 1.0), ((prev, last, Y), -1e8), ((last, Y), 1e8), ((last, 5 * per + 1), 3e8), ((5 * per + 1,), 2.0)]
    per_row = []
    for b in range(nb):                                                # a different subset applies in every row
        L = min(2 + b % 4, t)
        per_row.append((tuple(int(x) for x in ids[b, t - (L - 1):]) + (X if b % 2 else 7 * per + b,), 9.0 + b))
    out["per_row_subsets"] = list(dict(per_row).items())
    full = tuple(int(x) for x in ids[0])
    if t <= 15:
        out["L_is_t_and_t_plus_one"] = [(full[1:] + (X,), 50.0), (full + (Y,), 80.0)]       # L == t applies, L == t + 1 is skipped
    if t >= 15:
        out["length_16"] = [(full[t - 15:] + (X,), 50.0), (full[t - 15:-1] + (full[-1] + 1, Y), 80.0)]
    out["dead_tokens"] = [((v.notimestamps,), 90.0), ((v.sot,), 91.0), ((eos,), 92.0), ((tb + 1,), 93.5), ((2 * per + 5,), 95.25)]
    return out


def per_row_last(ids, V, per, X):
    """The last token of the sequence ``_tables`` lifts from each row for "per_row_subsets"."""
    return [X if b % 2 else 7 * per + b for b in range(len(ids))]


def _geometries(tiny, engines, large):
    g, v, W, spec = tiny
    return [("tiny", v, spec, engines["f32"]), ("large", large[1], large[2], large[3])]


@pytest.mark.parametrize("which", ["tiny", "large"])
def test_differential_on_the_sampler_cases(tiny, engines, large, which):
    """Every row of tests/sampler_cases.py (crafted grammar states, -inf logits, min_new_tokens) under tables that bias suppressed
    tokens, -inf logits, the eos under min_new_tokens, the slice edges and all 256 entries of one slice, in launches of up to 8."""
    name, v, spec, eng = dict((x[0], x) for x in _geometries(tiny, engines, large))[which]
    V = spec.vocab_size
    cs = SC.cases(v, V)
    groups = {}
    for i, (_, ids, lg, mn) in enumerate(cs):
        groups.setdefault((len(ids), mn), []).append(i)
    n = 0
    for (t, mn), idx in groups.items():
        for lo in range(0, len(idx), 8):
            sel = idx[lo:lo + 8]
            lg = np.stack([cs[i][2] for i in sel]); ids = np.stack([cs[i][1] for i in sel]).astype(np.int32)
            tabs = _tables(v, spec, V, ids)
            inf_tok = [int(np.flatnonzero(np.isneginf(lg[r]))[0]) for r in range(len(sel)) if np.isneginf(lg[r]).any()]
            if inf_tok:
                tabs["dead_tokens"] = tabs["dead_tokens"] + [((tok,), 70.0) for tok in sorted(set(inf_tok))]
            for tn, table in tabs.items():
                if which == "large" and tn not in ("dead_tokens", "slice_edges") and (lo > 0 or t % 3):
                    continue                                           # the float64 side costs milliseconds per row here: a third of the launches
                _differential(eng, spec, lg, ids, table, mn, what=f"{which} {tn} " + ",".join(cs[i][0] for i in sel))
            n += len(sel)
    assert n == len(cs) == 57


@pytest.mark.parametrize("nb", [1, 8])
@pytest.mark.parametrize("which", ["tiny", "large"])
def test_differential_on_crafted_tables(tiny, engines, large, which, nb):
    name, v, spec, eng = dict((x[0], x) for x in _geometries(tiny, engines, large))[which]
    V = spec.vocab_size
    _, per = geometry(V)
    for t_gen in (6, 15):                                              # t = 9, and t = 18 for the length-16 sequence
        ids, lg = _rows(v, spec, V, nb, 100 * nb + t_gen, t_gen)
        tabs = _tables(v, spec, V, ids)
        assert ("length_16" in tabs) == (t_gen == 15) and ("L_is_t_and_t_plus_one" in tabs) == (t_gen == 6)
        for tn, table in tabs.items():
            assert len(table) <= 256 and len(set(s for s, _ in table)) == len(table)
            lg2 = lg.copy()
            if tn == "dead_tokens":
                lg2[:, 2 * per + 5] = -np.inf
            got = _differential(eng, spec, lg2, ids, table, what=f"{which} nb={nb} t_gen={t_gen} {tn}")
            dense = S.dense_bias(ids, ids.shape[1], table, V)
            X, Y = (310, 311) if V > 2000 else (ord("x"), ord("y"))
            if tn == "slice_edges":
                assert got.tolist() == [V - 1] * nb                    # +60 on the last token of the last, partial float4 group
            elif tn == "order_dependent_sum":
                assert dense[0, X] == 0.0 and dense[0, Y] == 0.0 and dense[0, 5 * per + 1] == 3e8     # (1 + 1e8) - 1e8; 2 + 3e8
                assert got[0] == 5 * per + 1
            elif tn == "per_row_subsets":
                assert nb == 1 or len({dense[b].tobytes() for b in range(nb)}) >= 2     # the rows' subsets differ
                assert all(dense[b, table_last] != 0.0 for b, table_last in enumerate(per_row_last(ids, V, per, X)))
            elif tn == "L_is_t_and_t_plus_one":
                assert got[0] == X and dense[0, Y] == 0.0
            elif tn == "length_16":
                assert got[0] == X and dense[0, Y] == 0.0 and len(table[0][0]) == 16
            elif tn == "dead_tokens":
                assert v.notimestamps not in got.tolist() and v.sot not in got.tolist() and 2 * per + 5 not in got.tolist()
                assert spec.timestamp_begin + 1 not in got.tolist()    # below the floor set by the row's first timestamp


def test_a_bias_on_the_eos_under_min_new_tokens_and_the_timestamp_flip_and_the_demoted_winner(tiny, engines):
    g, v, W, spec = tiny
    eng = engines["f32"]
    V, tb, eos = spec.vocab_size, spec.timestamp_begin, spec.eos_token_id
    cs = {name: (ids, lg, mn) for name, ids, lg, mn in SC.cases(v, V)}
    # the eos stays masked under min_new_tokens whatever its bias
    ids, lg, mn = cs["after_text_ts_eos_masked_by_min_new_tokens"]
    got = _differential(eng, spec, lg[None], ids[None].astype(np.int32), [((eos,), 90.0)], mn, what="eos")
    assert mn > 0 and got[0] != eos
    free = _differential(eng, spec, lg[None], ids[None].astype(np.int32), [((eos,), 90.0)], 0, what="eos free")
    assert free[0] == eos
    # +2.0 on the two timestamp tokens of logsumexp_keeps_text: 2 * e^(3+2) > e^5, the rule now forces a timestamp
    ids, lg, mn = cs["logsumexp_keeps_text"]
    plain = eng.test_sample(lg[None], ids[None].astype(np.int32), 3)
    got = _differential(eng, spec, lg[None], ids[None].astype(np.int32), [((tb + 20,), 2.0), ((tb + 21,), 2.0)], what="flip")
    assert plain[0] < tb <= got[0] and got[0] == tb + 20
    # a negative bias demotes the winner of every row
    idx = [n for n in cs if n.startswith("random")][:8]
    for n in idx:
        ids, lg, mn = cs[n]
        plain = int(eng.test_sample(lg[None], ids[None].astype(np.int32), 3, min_new_tokens=mn)[0])
        got = _differential(eng, spec, lg[None], ids[None].astype(np.int32), [((plain,), -100.0)], mn, what="demote " + n)
        assert got[0] != plain


def test_the_c_entry_point_refuses_what_the_header_says(tiny, engines):
    g, v, W, spec = tiny
    eng = engines["f32"]
    V = spec.vocab_size
    A, B = ord("a"), ord("b")
    ok = [((A, B), 100.0)]
    ids, lg = _rows(v, spec, V, 1, 5)
    ids[0, -1] = A
    assert eng.test_sample(lg, ids, 3)[0] != B
    for bad, match in (([((V,), 1.0)], "outside"), ([((-1,), 1.0)], "outside"), ([((5,), float("inf"))], "finite"),
                       ([((5,), float("nan"))], "finite"), ([((5, 6), 1.0), ((5, 6), 2.0)], "same"),
                       ([(tuple(range(1, 18)), 1.0)], "tokens"), ([((i + 1,), 1.0) for i in range(257)], "sequences")):
        eng.set_sequence_bias(ok)
        with pytest.raises(Exception, match=match):
            eng.set_sequence_bias(bad)
        assert eng.test_sample(lg, ids, 3)[0] == B                     # refused before any state changed: the old table is in force
        assert eng.test_sample_biased(lg, ids, 3, K, None)[0][0] != B  # the hook's own (empty) table for one call ...
        assert eng.test_sample(lg, ids, 3)[0] == B                     # ... and the context's put back
        eng.set_sequence_bias(None)
        assert eng.test_sample(lg, ids, 3)[0] != B
    assert eng.lib.cw_set_sequence_bias(eng.ctx, 1, None, None, None) != 0                 # null pointers
    eng.set_sequence_bias([(tuple(range(1, 17)), 1.0)] + [((i + 1,), 1.0) for i in range(255)])   # exactly at the limits
    eng.mel(_clips(1))
    eng.encode([0], [0], [3000])
    try:
        with pytest.raises(Exception, match="sequence_bias"):
            eng.beam_begin(_prompt(v, 1), 2, 3 + 4)
    finally:
        eng.set_sequence_bias(None)


# ------------------------------------------------------------------------------------------------ real decodes of the tiny model
TEXT = 37                                                              # '%', the boosted byte of the golden's tables


def _dense_lp(spec, cap, seqs, lens, table, b):
    """float64: the processed-score log-probability of every token row b wrote, from the captured logits plus dense_bias."""
    V = spec.vocab_size
    out = []
    for t in range(3, int(lens[b])):
        x = cap[t - 3, b].astype(np.float32)
        xb = (x + S.dense_bias(seqs[b:b + 1, :t], t, table, V)[0]).astype(np.float32)
        s, _ = R.processed_scores(spec, xb, list(seqs[b, :t]), 3)
        m = s.max()
        out.append(s[int(seqs[b, t])] - (m + np.log(np.exp(s - m).sum())))
    return np.asarray(out, np.float64)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_real_decode_graph_and_plain_path_avg_logprob_and_off_on_off(tiny, engines, dt):
    g, v, W, spec = tiny
    eng = engines[dt]
    nb, steps, tb = 6, 14, spec.timestamp_begin
    _, nf = eng.mel(_clips(nb))
    eng.encode(list(range(nb)), [0] * nb, [3000] * nb)
    eng.set_thresholds(-1.0, None)
    eng.set_token_logprobs(True)
    bound = 2e-3 if dt == "f32" else 3e-2                              # tests/test_gpu_e2e.py, average log-probability

    def run(capture):
        cap = eng.capture_logits(nb, steps) if capture else None       # capturing takes the launch-per-kernel path
        try:
            seqs, lens, _ = eng.decode(_prompt(v, nb), max_length=3 + steps)
            cap = cap.copy() if capture else None
        finally:
            if capture:
                eng.stop_capture()
        return (seqs.copy(), lens.copy(), eng.avg_logprobs(nb).copy(), eng.token_timestamps(nb, int(lens.max()) - 1, 3, nf).copy(),
                eng.token_logprobs(nb).copy()), cap

    try:
        off, _ = run(False)
        first_text = int(off[0][0, 4])
        table = [((TEXT,), 6.0), ((first_text, TEXT), 30.0), ((int(v.transcribe), tb + 9), 25.0), ((tb + 100,), 3.0),
                 ((int(off[0][1, 3]), int(off[0][1, 4]), ord("z")), 40.0)]
        eng.set_sequence_bias(table)
        plain, cap = run(True)
        graph, _ = run(False)
        for a, b in zip(plain, graph):
            assert a.tobytes() == b.tobytes()
        seqs, lens, alp = plain[0], plain[1], plain[2]
        assert seqs.tobytes() != off[0].tobytes() and np.all(seqs[:, 3] == tb + 9)
        worst = 0.0
        for b in range(nb):
            want = _dense_lp(spec, cap, seqs, lens, table, b)
            worst = max(worst, abs(float(alp[b]) - float(want.mean())))
        print(f"{dt}: worst |avg_logprob - float64| = {worst:.3e} (bound {bound})")
        assert worst <= bound
        eng.set_sequence_bias(None)
        off2, _ = run(False)
        for a, b in zip(off, off2):
            assert a.tobytes() == b.tobytes()
    finally:
        eng.set_sequence_bias(None)
        eng.set_token_logprobs(False)
        eng.set_thresholds(None, None)


def test_native_seek_loop_equals_host_loop(tiny, engines):
    g, v, W, spec = tiny
    eng = engines["f32"]
    clips = [syn.synth_audio(60 + i, n, kind) for i, (n, kind) in
             enumerate([(480000, "mixed"), (130000, "noise"), (300001, "chirp"), (1600, "noise")])]
    _, nf = eng.mel(clips)
    kw = dict(language="<|en|>", task="transcribe", max_new_tokens=40)
    table = [[[TEXT], 4.0], [[ord("a"), TEXT], 30.0], [[int(v.transcribe), spec.timestamp_begin + 4], 30.0]]
    sa, sb = {}, {}
    a = generation.generate(eng, len(clips), nf, stats=sa, native=True, sequence_bias=table, **kw)
    b = generation.generate(eng, len(clips), nf, stats=sb, native=False, sequence_bias=table, **kw)
    plain = generation.generate(eng, len(clips), nf, native=True, **kw)
    again = generation.generate(eng, len(clips), nf, native=False, **kw)
    assert sa == sb and sa["generate_calls"] > 1
    assert np.array_equal(a["sequences"], b["sequences"]) and not np.array_equal(a["sequences"], plain["sequences"])
    assert np.array_equal(plain["sequences"], again["sequences"])      # the table did not outlive its call
    for i in range(len(clips)):
        assert a["token_timestamps"][i].tobytes() == b["token_timestamps"][i].tobytes()
    assert all(int(s[0]) == spec.timestamp_begin + 4 for s in a["sequences"])


def test_fallback_redecodes_keep_the_table(tiny):
    """Temperatures (0, 0.5, 0.9) and a compression-ratio threshold every decode fails: three decodes of the window, each under the
    table.  Every token of every decode is the float64 arg-max of the (perturbed) processed scores of captured logits + dense_bias."""
    g, v, W, spec = tiny
    eng = Engine(spec, dtype="f32", max_batch=2)
    try:
        eng.load_state_dict(W)
        x = syn.synth_audio(4, 20 * 16000, "mixed")
        _, nf = eng.mel([x])
        eng.encode([0], [0], [3000])
        temps, seed, steps = (0.0, 0.5, 0.9), 99, 8
        tb = spec.timestamp_begin
        table = [((TEXT,), 3.0), ((tb + 30, TEXT), 12.0), ((int(v.transcribe), tb + 30), 20.0), ((ord("b"),), -4.0)]
        init = _prompt(v, 1)
        eng.set_sequence_bias(table)
        cap = eng.capture_logits(1, steps)
        records = []
        orig = eng.decode

        def spy(*a, **kw):
            out = orig(*a, **kw)
            records.append((cap.copy(), out[0].copy(), out[1].copy()))
            return out

        eng.decode = spy
        st = {}
        try:
            generation._decode_with_fallback(eng, spec, {"temps": temps, "seed": seed, "item_ids": [0], "cr_thr": 0.05}, [0], init, 3,
                                             3 + steps, 0, np.asarray(nf, np.int64), np.array([0]), None, None, None, st)
        finally:
            eng.decode = orig
            eng.stop_capture()
        assert [r["temperature_index"] for r in st["fallback"]] == [0, 1, 2] and len(records) == 3
        n = n_close = 0
        for ti, (c, seqs, lens) in enumerate(records):
            assert seqs[0, 3] == tb + 30                               # the prompt-anchored entry, at every temperature
            for t in range(3, int(lens[0])):
                xb = (c[t - 3, 0].astype(np.float32) + S.dense_bias(seqs[:1, :t], t, table, spec.vocab_size)[0]).astype(np.float32)
                tok = int(seqs[0, t])
                if temps[ti] == 0.0:
                    s, _ = R.processed_scores(spec, xb, list(seqs[0, :t]), 3)
                    top = np.sort(s)[-2:]
                    res = "ok" if tok == int(np.argmax(s)) else ("close" if top[1] - top[0] < 1e-5 else "wrong")
                else:
                    res, detail = R.check_token(spec, xb, list(seqs[0, :t]), 3, tok, temps[ti], seed, stream_id(0, 0, ti))
                assert res != "wrong", (ti, t, tok)
                n += 1
                n_close += res == "close"
        assert n >= 3 * 4 and n_close <= 1, (n, n_close)
        assert records[1][1].tobytes() != records[0][1].tobytes()
    finally:
        eng.set_sequence_bias(None)
        eng.close()


# ------------------------------------------------------------------------------------------------ transformers and the pipeline
def _pipe(tiny, batch_size=1, **kw):
    g, v, W, spec = tiny
    return cw.pipeline("automatic-speech-recognition", model=cw.ModelBundle(spec, W), tokenizer=collate.Vocabulary.from_synthetic(v),
                       chunk_length_s=30, batch_size=batch_size, return_timestamps="word", torch_dtype="float32",
                       device="cuda:0", num_beams=1, **kw)


def _spy(monkeypatch):
    recorded = []
    orig = generation.generate

    def spy(*a, **kw):
        out = orig(*a, **kw)
        recorded.append((list(kw["item_ids"]), out, kw))
        return out

    monkeypatch.setattr(generation, "generate", spy)
    return recorded


def test_against_transformers_f32(tiny, monkeypatch):
    """transformers' own greedy ids under six tables on six clips (tests/golden/gen_golden_sequence_bias.py: every case differs
    from its baseline and holds a gap above GOLD_GAP between its two best processed scores at every step), through pipe(...)."""
    g, v, W, spec = tiny
    assert GOLD["init"] == [v.sot, v.lang_id("en"), v.transcribe] and GOLD["gap"] == GOLD_GAP
    assert len(GOLD["cases"]) == 36 and len({c["name"] for c in GOLD["cases"]}) == 6
    pipe = _pipe(tiny)
    rec = _spy(monkeypatch)
    try:
        for c in GOLD["cases"]:
            assert c["ids"] != c["baseline"] and c["min_gap"] > GOLD_GAP
            x = syn.synth_audio(c["clip"]["seed"], int(round(c["clip"]["secs"] * 16000)), c["clip"]["kind"])
            del rec[:]
            pipe(x, generate_kwargs={"num_beams": 1, "language": "<|en|>", "task": "transcribe", "max_new_tokens": c["max_new_tokens"],
                                     "sequence_bias": c["sequence_bias"]})
            assert len(rec) == 1
            out = rec[0][1]
            n = len(out["token_timestamps"][0])
            assert out["sequences"][0][:n].tolist() == c["ids"], (c["clip"], c["name"])
    finally:
        pipe.engine.close()


def test_pipeline_short_clip_long_clip_prompt_and_refusals(tiny, monkeypatch):
    g, v, W, spec = tiny
    tb = spec.timestamp_begin
    gk = {"language": "<|en|>", "task": "transcribe", "max_new_tokens": 6, "num_beams": 1}
    pipe = _pipe(tiny, batch_size=2)
    rec = _spy(monkeypatch)
    try:
        # a short clip: the words change to what transformers' ids under the table spell
        case = next(c for c in GOLD["cases"] if c["name"] == "single_token")
        x = syn.synth_audio(case["clip"]["seed"], int(round(case["clip"]["secs"] * 16000)), case["clip"]["kind"])
        base = pipe(x, generate_kwargs=dict(gk))
        got = pipe(x, generate_kwargs=dict(gk, sequence_bias=case["sequence_bias"]))
        assert case["ids"][1:] == [TEXT] * 5 and got["text"] == "%%%%%" != base["text"]
        assert "".join(w["text"] for w in got["chunks"]) == "%%%%%"
        assert pipe(x, generate_kwargs=dict(gk)) == base               # nothing stays behind
        # 70 s in windows of 30 s: every window decodes under the table
        long = syn.synth_audio(0, 70 * 16000, "mixed")
        del rec[:]
        pipe(long, generate_kwargs=dict(gk, sequence_bias=[[[TEXT], 30.0]]))
        n_win = 0
        for idxs, out, kw in rec:
            assert kw["sequence_bias"] == [[[TEXT], 30.0]]
            for j in range(len(idxs)):
                n = len(out["token_timestamps"][j])
                toks = out["sequences"][j][:n]
                assert n >= 2 and np.all(toks[toks < tb] == TEXT) and np.any(toks < tb)
                n_win += 1
        assert n_win == len(audio.chunk_windows(len(long), 480000, 80000, 80000)) == 3
        # prompt_ids: a sequence whose prefix ends in the prompt's last tokens applies at the first generated position
        prompt = np.array([v.startofprev, ord("h"), ord("i")], np.int64)
        init = [int(v.sot), int(v.lang_id("en")), int(v.transcribe)]
        first = {}
        for name, head in (("into_prompt", ord("i")), ("other", ord("j"))):
            del rec[:]
            pipe(x, generate_kwargs=dict(gk, prompt_ids=prompt, sequence_bias=[[[head] + init + [tb + 33], 40.0]]))
            first[name] = int(rec[0][1]["sequences"][0][0])
        del rec[:]
        pipe(x, generate_kwargs=dict(gk, prompt_ids=prompt))
        assert first["into_prompt"] == tb + 33 != first["other"] == int(rec[0][1]["sequences"][0][0])
        # refusals: before anything runs, and nothing stays behind
        del rec[:]
        with pytest.raises(ValueError, match="num_beams': 1"):
            pipe(x, generate_kwargs=dict(gk, num_beams=5, sequence_bias=[[[TEXT], 30.0]]))
        for who in ("align", "score"):
            with pytest.raises(ValueError, match="sequence_bias"):
                getattr(pipe, who)(x, [ord("a"), ord("b")], sequence_bias=[[[TEXT], 30.0]])
        assert rec == [] and pipe(x, generate_kwargs=dict(gk)) == base
    finally:
        pipe.engine.close()
