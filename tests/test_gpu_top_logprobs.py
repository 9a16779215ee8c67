"""top_logprobs (cw_set_top_logprobs; sample_partial_kernel<true> / sample_kernel<T, true> in csrc/elementwise.hip) on the device:
ids exactly those of float64 on the logits of the very step and values within the bound derived in tests/token_logprob_refs.py
(comparator and crafted rows: tests/top_logprob_refs.py), the -1 / NaN pattern, the captured-graph path, masked rows, the switch
leaving every existing output alone, the native seek loop against the host loop, transformers' own ranking, and the pipeline's
per-word "tokens"."""
import numpy as np
import pytest

import crisperwhisper_amd as cw
from crisperwhisper_amd import audio, collate, generation, synthetic as syn
from crisperwhisper_amd.engine import Engine
from crisperwhisper_amd.generation import stream_id
from crisperwhisper_amd.pipeline import token_text
from tests import helpers as Hh
from tests import sampler_cases as SC
from tests import token_logprob_refs as R
from tests import top_logprob_refs as T
from tests.top_logprob_refs import GOLD_GAP as GAP, GOLD_K as K_TEST, GOLD_MAX_LEFT_OUT as MAX_LEFT_OUT, checked_pairs
from tests.test_gpu_score_vs_transformers import BOUND
from tests.test_gpu_token_logprobs import _clips, _prompt, _random_rows

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "bf16", "f16"]
GOLD = Hh.gold_json("top_logprobs_golden.json")


@pytest.fixture(scope="module")
def tiny():
    return Hh.tiny_setup()


@pytest.fixture(scope="module")
def engines(tiny):
    g, v, W, spec = tiny
    out = {}
    for dt in DTYPES:
        e = Engine(spec, dtype=dt, max_batch=64)
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
    eng = Engine(spec, dtype="bf16", max_batch=64)
    yield g, v, spec, eng
    eng.close()


def _same_bits_where_written(tok, lp, top_id, top_lp):
    """Where the written token is among the alternatives its value is the token log-probability, bit for bit."""
    n = 0
    for b in range(len(tok)):
        j = np.flatnonzero(top_id[b] == int(tok[b]))
        assert len(j) <= 1
        if len(j):
            assert top_lp[b, j[0]].tobytes() == lp[b].tobytes(), (b, int(tok[b]), float(top_lp[b, j[0]]), float(lp[b]))
            n += 1
    return n


def _hook(eng, V, logits, ids, k, temp, seed, streams, forced=None, min_new=0, what=""):
    """The hook: its choice held against the existing hooks', its token value against the token hook's, ids and values against
    float64.  Returns (written token, token logprob, top ids, top logprobs)."""
    st = streams if temp > 0 else None
    choice, lp, top_id, top_lp = eng.test_sample_top_logprobs(logits, ids, 3, k, temp, seed, st, forced=forced, min_new_tokens=min_new)
    assert top_id.shape == top_lp.shape == (len(logits), k) and top_id.dtype == np.int32 and top_lp.dtype == np.float32
    choice0, lp0 = eng.test_sample_logprobs(logits, ids, 3, temp, seed, st, forced=forced, min_new_tokens=min_new)
    if temp > 0:
        want = eng.test_sample_seeded(logits, ids, 3, temp, seed, streams, min_new_tokens=min_new)
    else:
        want = eng.test_sample(logits, ids, 3, min_new_tokens=min_new)
    assert choice.tolist() == want.tolist() == choice0.tolist()
    assert lp.tobytes() == lp0.tobytes()                        # the alternatives leave the token's own value alone
    T.check_topk_rows(top_id, top_lp, logits, V, k, what=what)
    tok = choice.copy() if forced is None else np.where(np.asarray(forced) >= 0, forced, choice)
    _same_bits_where_written(tok, lp, top_id, top_lp)
    return tok, lp, top_id, top_lp


@pytest.mark.parametrize("temp", [0.0, 0.6])
@pytest.mark.parametrize("k", [1, 5, 8])
@pytest.mark.parametrize("dt", DTYPES)
def test_hook_on_the_sampler_cases(tiny, engines, dt, k, temp):
    """The 57 crafted and random rows of tests/sampler_cases.py, in launches of up to four rows sharing (t, min_new_tokens)."""
    g, v, W, spec = tiny
    eng = engines[dt]
    cs = SC.cases(v, v.size)
    assert len(cs) == 57
    groups = {}
    for i, (name, ids, lg, mn) in enumerate(cs):
        groups.setdefault((len(ids), mn), []).append(i)
    n = hits = 0
    for (t, mn), idx in groups.items():
        for lo in range(0, len(idx), 4):
            sel = idx[lo:lo + 4]
            lg = np.stack([cs[i][2] for i in sel]); ids = np.stack([cs[i][1] for i in sel])
            tok, lp, top_id, top_lp = _hook(eng, spec.vocab_size, lg, ids, k, temp, 77 + lo, [stream_id(i, 0, 1) for i in sel],
                                            min_new=mn, what=f"{dt} k={k} T={temp} " + ",".join(cs[i][0] for i in sel))
            hits += int(sum(int(tok[b]) in top_id[b] for b in range(len(sel))))
            n += len(sel)
    assert n == 57
    print(f"{dt} k={k} T={temp}: the written token is among the alternatives in {hits} of {n} rows")
    assert hits > 0


@pytest.mark.parametrize("temp", [0.0, 0.6])
@pytest.mark.parametrize("k", [1, 5, 8])
@pytest.mark.parametrize("nb", [1, 8, 64])
@pytest.mark.parametrize("dt", DTYPES)
def test_hook_on_random_rows_tiny_vocabulary(tiny, engines, dt, nb, k, temp):
    """V = 1769: one float4 group per thread, three pad columns (the hook holds +75 there)."""
    g, v, W, spec = tiny
    eng = engines[dt]
    assert spec.vocab_size == 1769 and R.n_iter(spec.vocab_size) == 1
    rng = np.random.default_rng(1000 * nb + 10 * k + int(temp * 10))
    for name, hist, lg, forced in _random_rows(rng, nb, spec.vocab_size, spec.timestamp_begin, spec.eos_token_id, ord("a")):
        ids = np.tile(np.array([v.sot, v.lang_id("en"), v.transcribe] + hist, np.int32), (nb, 1))
        _hook(eng, spec.vocab_size, lg, ids, k, temp, 5 + nb, [stream_id(b, 10 * b, 2) for b in range(nb)], forced=forced,
              what=f"{dt} nb={nb} k={k} T={temp} {name}")


@pytest.mark.parametrize("temp", [0.0, 0.6])
@pytest.mark.parametrize("nb, k", [(1, 5), (8, 8), (64, 1), (64, 8)])
def test_hook_on_random_rows_large_vocabulary(large, nb, k, temp):
    """V = 51866: four groups per thread, the last slice short.  The float64 side costs 2 ms per value here, so 64 rows x 8 ranks
    look at the two row kinds that differ most (spread, dominant last id forced) and the narrower launches at all five."""
    g, v, spec, eng = large
    V = spec.vocab_size
    assert V == 51866 and V % 4 and R.n_iter(V) == 4
    rng = np.random.default_rng(2000 * nb + 10 * k + int(temp * 10))
    rows = _random_rows(rng, nb, V, spec.timestamp_begin, spec.eos_token_id, 300)
    if nb * k > 64:
        rows = [r for r in rows if r[0] in ("spread", "dominant_last_id_forced")]
        assert len(rows) == 2
    for name, hist, lg, forced in rows:
        ids = np.tile(np.array([v.sot, v.lang_id("en"), v.transcribe] + hist, np.int32), (nb, 1))
        _hook(eng, V, lg, ids, k, temp, 9 + nb, [stream_id(b, 10 * b, 2) for b in range(nb)], forced=forced,
              what=f"V={V} nb={nb} k={k} T={temp} {name}")


def _crafted(eng, v, spec, k, temp, what):
    V = spec.vocab_size
    rows = T.crafted_rows(V, k)
    names = [r[0] for r in rows]
    lg = np.stack([r[1][:V] for r in rows])                    # the hook itself holds +75 in the pad columns
    nb = len(rows)
    ids = np.tile(np.array([v.sot, v.lang_id("en"), v.transcribe, spec.timestamp_begin + 3, 300 if V > 2000 else ord("a")], np.int32), (nb, 1))
    streams = [stream_id(b, 7 * b, 1) for b in range(nb)]
    tok, lp, top_id, top_lp = _hook(eng, V, lg, ids, k, temp, 31, streams, what=what)
    want = [T.reference_topk(x, V, k)[0] for x in lg]
    # what the rows are for, spelled out: the tie rows list their tied ids in ascending order, ...
    _, per = T.geometry(V)
    tie = want[names.index("tie_across_slice_boundary")]
    assert tie[:min(k, 3)].tolist() == [per - 1, per, 2 * per][:min(k, 3)] and top_id[0].tolist() == tie.tolist()
    # ... the last ids of the vocabulary are listed and no pad column ever is, ...
    last = names.index("winners_in_the_last_float4")
    assert top_id[last, :min(k, 3)].tolist() == [V - 2, V - 3, V - 1][:min(k, 3)] and np.all(top_id < V)
    # ... fewer than k finite logits leave -1 / NaN behind them, ...
    few = names.index("fewer_than_k_finite")
    n_fin = max(k - 2, 0)
    assert np.all(top_id[few, :n_fin] >= 0) and np.all(top_id[few, n_fin:] == -1) and np.all(np.isnan(top_lp[few, n_fin:]))
    # ... and a NaN logit is never listed
    nan = names.index("nan_logit")
    bad = int(np.flatnonzero(np.isnan(lg[nan]))[0])
    assert bad not in top_id[nan].tolist() and np.all(top_id[nan] >= 0)
    # a forced token outside the top k: the alternatives stay, the token's own value is the forced token's
    forced = np.full(nb, -1, np.int32)
    for b in range(nb):
        fin = np.flatnonzero(np.isfinite(lg[b]) & ~np.isin(np.arange(V), want[b]))
        if len(fin):
            forced[b] = fin[np.argmin(lg[b][fin])]
    assert np.sum(forced >= 0) >= nb - 2
    tok2, lp2, top_id2, top_lp2 = _hook(eng, V, lg, ids, k, temp, 31, streams, forced=forced, what=what + " forced")
    assert top_id2.tobytes() == top_id.tobytes() and top_lp2.tobytes() == top_lp.tobytes()
    sel = np.flatnonzero(forced >= 0)
    assert all(int(tok2[b]) == int(forced[b]) and int(forced[b]) not in top_id2[b] for b in sel)
    live = [b for b in sel if b != nan]
    R.check_rows(lp2[live], lg[live], forced[live], V, what=what + " forced token's own value")


@pytest.mark.parametrize("temp", [0.0, 0.6])
@pytest.mark.parametrize("k", [1, 5, 8])
@pytest.mark.parametrize("dt", DTYPES)
def test_crafted_rows_tiny_vocabulary(tiny, engines, dt, k, temp):
    g, v, W, spec = tiny
    _crafted(engines[dt], v, spec, k, temp, f"crafted {dt} k={k} T={temp}")


@pytest.mark.parametrize("temp", [0.0, 0.6])
@pytest.mark.parametrize("k", [1, 5, 8])
def test_crafted_rows_large_vocabulary(large, k, temp):
    g, v, spec, eng = large
    assert T.geometry(spec.vocab_size)[1] > 256 * 4              # wave boundaries and several groups per thread exist here
    _crafted(eng, v, spec, k, temp, f"crafted V={spec.vocab_size} k={k} T={temp}")


def test_the_c_entry_points_refuse_what_the_header_says(tiny, engines):
    g, v, W, spec = tiny
    eng = engines["f32"]
    with pytest.raises(Exception, match="token log-probabilities"):
        eng.set_top_logprobs(3)                                 # token log-probabilities are off
    eng.set_top_logprobs(0)                                     # off while off: fine
    eng.set_token_logprobs(True)
    try:
        for bad in (-1, 9):
            with pytest.raises(Exception, match="outside"):
                eng.set_top_logprobs(bad)
        with pytest.raises(Exception, match="off"):
            eng.top_logprobs(1)
        eng.set_top_logprobs(8)
        ids, lps = eng.top_logprobs(2)
        assert ids.shape == lps.shape == (2, spec.max_target_positions, 8)
        assert np.all(ids == -1) and np.all(np.isnan(lps))      # nothing decoded under the switch yet
        eng.set_token_logprobs(False)                           # ... switches the alternatives off as well
        eng.set_token_logprobs(True)
        with pytest.raises(Exception, match="off"):
            eng.top_logprobs(1)
    finally:
        eng.set_token_logprobs(False)


def _decode(eng, v, nb, steps, temp, forced=None, capture=False, row_active=None):
    if temp > 0:
        eng.set_sampling(temp, 4242 + nb, [stream_id(b, 0, 3) for b in range(nb)])
    cap = eng.capture_logits(nb, steps) if capture else None
    try:
        seqs, lens, _ = eng.decode(_prompt(v, nb), max_length=3 + steps, forced=forced, row_active=row_active)
        cap = cap.copy() if capture else None
    finally:
        if capture:
            eng.stop_capture()
        eng.set_sampling(0.0)
    return seqs, lens, cap, eng.token_logprobs(nb), eng.top_logprobs(nb)


@pytest.mark.parametrize("temp", [0.0, 0.6])
@pytest.mark.parametrize("nb", [1, 8, 17])
@pytest.mark.parametrize("dt", DTYPES)
def test_real_decode_against_float64_on_the_captured_logits(tiny, engines, dt, nb, temp):
    """Free-running, and with an eos forced at a different position per row so that rows end inside the decode: at every generated
    position (the eos included) ids exact and values bounded against float64 on the logits of its own step, -1 / NaN exactly
    where the token log-probability is NaN; the same decode through the captured step graph gives the same bytes."""
    g, v, W, spec = tiny
    eng = engines[dt]
    steps, V, tgt, k = 10, spec.vocab_size, spec.max_target_positions, 5
    eng.mel(_clips(nb))
    eng.encode(list(range(nb)), [0] * nb, [3000] * nb)
    eng.set_token_logprobs(True)
    eng.set_top_logprobs(k)
    try:
        forced = np.full((nb, 3 + steps), -1, np.int32)
        for b in range(nb):
            forced[b, 3 + 2 + b % 6] = spec.eos_token_id
        for fr in (None, forced):
            seqs, lens, cap, lp, (tid, tlp) = _decode(eng, v, nb, steps, temp, forced=fr, capture=True)
            assert tid.shape == tlp.shape == (nb, tgt, k) and tid.dtype == np.int32 and tlp.dtype == np.float32
            none = np.isnan(lp)
            assert np.all(tid[none] == -1) and np.all(np.isnan(tlp[none]))
            assert np.all(tid[~none] >= 0) and not np.any(np.isnan(tlp[~none]))       # V finite logits: all k ranks exist
            worst = 0.0
            for b in range(nb):
                L = int(lens[b])
                assert not np.any(none[b, 3:L]) and np.all(none[b, :3]) and np.all(none[b, L:])
                for t in range(3, L):
                    ok, w, why = T.compare_topk(tid[b, t], tlp[b, t], cap[t - 3, b], V, k)
                    assert ok, (dt, nb, temp, fr is not None, b, t, why)
                    worst = max(worst, w)
                _same_bits_where_written(seqs[b, 3:L], lp[b, 3:L], tid[b, 3:L], tlp[b, 3:L])
            print(f"{dt} nb={nb} T={temp} forced={fr is not None}: worst |err| / bound = {worst:.3f}")
            seqs2, lens2, _, lp2, (tid2, tlp2) = _decode(eng, v, nb, steps, temp, forced=fr, capture=False)   # captured step graph
            assert seqs2.tobytes() == seqs.tobytes() and lens2.tobytes() == lens.tobytes() and lp2.tobytes() == lp.tobytes()
            assert tid2.tobytes() == tid.tobytes() and tlp2.tobytes() == tlp.tobytes()
    finally:
        eng.set_token_logprobs(False)


def test_a_masked_row_keeps_its_entries(tiny, engines):
    g, v, W, spec = tiny
    eng = engines["f32"]
    nb, steps = 4, 12
    eng.mel(_clips(nb))
    eng.encode(list(range(nb)), [0] * nb, [3000] * nb)
    eng.set_token_logprobs(True)
    eng.set_top_logprobs(5)
    try:
        s0, l0, _, lp0, (tid0, tlp0) = _decode(eng, v, nb, steps, 0.0)
        mask = np.array([1, 0, 1, 0], np.int32)
        s1, l1, _, lp1, (tid1, tlp1) = _decode(eng, v, nb, steps - 4, 0.8, row_active=mask)
        assert l1[1] == 0 and l1[3] == 0
        for b in (1, 3):
            assert np.any(tid0[b] >= 0)
            assert tid1[b].tobytes() == tid0[b].tobytes() and tlp1[b].tobytes() == tlp0[b].tobytes()
        for b in (0, 2):
            L = int(l1[b])
            none = np.isnan(lp1[b])
            assert np.all(none[:3]) and np.all(none[L:]) and not np.any(none[3:L])
            assert np.all(tid1[b][none] == -1) and np.all(np.isnan(tlp1[b][none])) and np.all(tid1[b][~none] >= 0)
        far = eng.top_logprobs(8)                               # rows never decoded under the switch
        assert np.all(far[0][nb:] == -1) and np.all(np.isnan(far[1][nb:]))
    finally:
        eng.set_token_logprobs(False)
    with pytest.raises(Exception):
        eng.top_logprobs(nb)                                    # off: refused, not stale


@pytest.mark.parametrize("dt", DTYPES)
def test_the_switch_changes_no_existing_output(tiny, dt):
    """k = 0 / 5 / 0: sequences, lengths, average log-probabilities, token timestamps and token log-probabilities byte for byte."""
    g, v, W, spec = tiny
    eng = Engine(spec, dtype=dt, max_batch=8)
    try:
        eng.load_state_dict(W)
        nb = 6
        _, nf = eng.mel(_clips(nb))
        eng.encode(list(range(nb)), [0] * nb, [3000] * nb)
        eng.set_thresholds(-1.0, None)
        eng.set_token_logprobs(True)

        def run(temp):
            if temp > 0:
                eng.set_sampling(temp, 3, [stream_id(b, 0, 2) for b in range(nb)])
            try:
                seqs, lens, _ = eng.decode(_prompt(v, nb), max_length=3 + 20)
            finally:
                eng.set_sampling(0.0)
            return (seqs.copy(), lens.copy(), eng.avg_logprobs(nb).copy(),
                    eng.token_timestamps(nb, int(lens.max()) - 1, 3, nf).copy(), eng.token_logprobs(nb).copy())

        for temp in (0.0, 0.6):
            off = run(temp)
            eng.set_top_logprobs(5)
            on = run(temp)
            assert np.any(eng.top_logprobs(nb)[0] >= 0)
            eng.set_top_logprobs(0)
            off2 = run(temp)
            for a, b, c in zip(off, on, off2):
                assert a.tobytes() == b.tobytes() == c.tobytes()
    finally:
        eng.close()


def test_native_seek_loop_equals_host_loop(tiny, engines):
    g, v, W, spec = tiny
    eng = engines["f32"]
    clips = [syn.synth_audio(60 + i, n, kind) for i, (n, kind) in
             enumerate([(480000, "mixed"), (130000, "noise"), (300001, "chirp"), (1600, "noise")])]
    _, nf = eng.mel(clips)
    sa, sb = {}, {}
    k = 5
    kw = dict(language="<|en|>", task="transcribe", max_new_tokens=40, return_token_logprobs=True)
    a = generation.generate(eng, len(clips), nf, stats=sa, native=True, top_logprobs=k, **kw)
    b = generation.generate(eng, len(clips), nf, stats=sb, native=False, top_logprobs=k, **kw)
    plain = generation.generate(eng, len(clips), nf, native=True, **kw)
    assert sa == sb and sa["generate_calls"] > 1                      # a multi-pass clip
    assert "top_ids" not in plain and "top_logprobs" not in plain
    assert np.array_equal(plain["sequences"], a["sequences"]) and np.array_equal(a["sequences"], b["sequences"])
    for i in range(len(clips)):
        n = len(a["token_timestamps"][i])
        assert a["token_logprobs"][i].tobytes() == b["token_logprobs"][i].tobytes() == plain["token_logprobs"][i].tobytes()
        for key, dtype in (("top_ids", np.int32), ("top_logprobs", np.float32)):
            assert a[key][i].dtype == dtype and b[key][i].dtype == dtype and a[key][i].shape == b[key][i].shape == (n, k)
            assert a[key][i].tobytes() == b[key][i].tobytes()
        assert np.all(a["top_ids"][i] >= 0) and np.all(a["top_ids"][i] < spec.vocab_size) and not np.any(np.isnan(a["top_logprobs"][i]))
        assert np.all(np.diff(a["top_logprobs"][i], axis=1) <= 0)     # best first
        _same_bits_where_written(a["sequences"][i][:n], a["token_logprobs"][i], a["top_ids"][i], a["top_logprobs"][i])
    for segs, ti in zip(b["segments"], b["top_ids"]):
        assert sum(len(s.top_ids) for s in segs) == len(ti) and all(s.top_logprobs.shape == s.top_ids.shape for s in segs)


def test_against_transformers_f32(tiny, engines):
    """The f32 engine's free-running greedy decode with k = 5 against transformers' own ranking of the same steps
    (tests/golden/gen_golden_top_logprobs.py): rank j is held to the golden -- id equal, value within BOUND["float32"] -- where both
    of its neighbour gaps in the golden exceed twice that bound; the pairs that fail the gap test are left out, at most 10 % of
    them.  (The 16-bit engines' bounds, 0.08 / 0.5, are wider than the gaps between neighbours: they are held to float64 on their
    own logits by the tests above.)"""
    g, v, W, spec = tiny
    eng = engines["f32"]
    bound = BOUND["float32"]
    assert GOLD["init"] == [v.sot, v.lang_id("en"), v.transcribe] and GOLD["k"] == K_TEST == 5 and GOLD["n_top"] == 6
    assert GAP == GOLD["gap"] == 2 * bound == 8e-3 and MAX_LEFT_OUT == GOLD["max_left_out"] == 0.10
    n_pairs = n_checked = 0
    worst = 0.0
    for c in GOLD["cases"]:
        ids = np.asarray(c["ids"], np.int64)
        ref_id, ref_lp = np.asarray(c["top_ids"], np.int64), np.asarray(c["top_logprobs"], np.float64)
        x = syn.synth_audio(c["clip"]["seed"], int(round(c["clip"]["secs"] * 16000)), c["clip"]["kind"])
        _, nf = eng.mel([x])
        out = generation.generate(eng, 1, nf, language="<|en|>", task="transcribe", max_new_tokens=c["max_new_tokens"],
                                  num_beams=1, return_token_logprobs=True, top_logprobs=K_TEST)
        assert out["sequences"][0].tolist() == ids.tolist(), c["clip"]
        got_id, got_lp = out["top_ids"][0], out["top_logprobs"][0]
        assert got_id.shape == got_lp.shape == (len(ids), K_TEST)
        ok = checked_pairs(ref_lp, K_TEST, GAP)
        n_pairs += ok.size; n_checked += int(ok.sum())
        d = np.abs(got_lp.astype(np.float64) - ref_lp[:, :K_TEST])
        print(c["clip"]["seed"], "checked", int(ok.sum()), "of", ok.size, "max |logprob - ref| =", float(d[ok].max()))
        worst = max(worst, float(d[ok].max()))
        assert np.array_equal(got_id[ok], ref_id[:, :K_TEST][ok]), (c["clip"], got_id.tolist(), ref_id.tolist())
        assert np.all(d[ok] <= bound), (c["clip"], float(d[ok].max()))
    print("left out", n_pairs - n_checked, "of", n_pairs, "worst", worst, "bound", bound)
    assert n_pairs - n_checked <= MAX_LEFT_OUT * n_pairs


@pytest.mark.parametrize("call", ["greedy", "prompt", "fallback"])
def test_pipeline_word_tokens(tiny, call, monkeypatch):
    """The 70 s clip of test_pipeline_word_logprobs with strides at batch 2: the chunks' text, timestamp and logprob are those of
    the call without top_logprobs, and every word's "tokens" are generate's arrays over the collator's groups; 5 beams raise."""
    g, v, W, spec = tiny
    x = syn.synth_audio(0, 70 * 16000, "mixed")
    gk = {"language": "<|en|>", "task": "transcribe", "max_new_tokens": 16, "num_beams": 1}
    if call == "prompt":
        gk["prompt_ids"] = np.array([v.startofprev, ord("h"), ord("i")], np.int64)
    elif call == "fallback":
        gk.update(temperature=(0.0, 0.6), compression_ratio_threshold=1.2, logprob_threshold=-1.0)
    k = 5
    pipe = cw.pipeline("automatic-speech-recognition", model=cw.ModelBundle(spec, W), tokenizer=collate.Vocabulary.from_synthetic(v),
                       chunk_length_s=30, batch_size=2, return_timestamps="word", torch_dtype="float32", device="cuda:0",
                       sampling_seed=11, return_scores=True)
    try:
        scored = pipe(x, generate_kwargs=dict(gk))
        assert all("tokens" not in w for w in scored["chunks"])
        recorded = []
        orig = generation.generate

        def spy(*a, **kw):
            out = orig(*a, **kw)
            recorded.append((list(kw["item_ids"]), out))
            return out

        monkeypatch.setattr(generation, "generate", spy)
        top = pipe(x, generate_kwargs=dict(gk), top_logprobs=k)
        monkeypatch.undo()
        assert top["text"] == scored["text"] and len(top["chunks"]) > 3
        assert [{n: w[n] for n in ("text", "timestamp", "logprob")} for w in top["chunks"]] == scored["chunks"]
        assert all(set(w) == {"text", "timestamp", "logprob", "tokens"} for w in top["chunks"])
        windows = audio.chunk_windows(len(x), 480000, 80000, 80000)
        assert len(windows) == 3 and len(recorded) == 2
        outputs, per = {}, {}
        for idxs, out in recorded:
            for j, i in enumerate(idxs):
                n = len(out["token_timestamps"][j])
                assert out["top_ids"][j].shape == out["top_logprobs"][j].shape == (n, k)
                outputs[i] = {"tokens": out["sequences"][j][:n], "token_timestamps": out["token_timestamps"][j],
                              "stride": tuple(t / 16000 for t in windows[i][2])}
                per[i] = (out["token_logprobs"][j], out["top_ids"][j], out["top_logprobs"][j])
        order = sorted(outputs)
        text, words, groups = collate.decode_asr(pipe.vocab, [dict(outputs[i]) for i in order], return_timestamps="word",
                                                 return_token_groups=True)
        toks = np.concatenate([outputs[i]["tokens"] for i in order])
        lp = np.concatenate([per[i][0] for i in order]); tid = np.concatenate([per[i][1] for i in order])
        tlp = np.concatenate([per[i][2] for i in order])
        assert text == top["text"] and len(words) == len(top["chunks"])
        n_alt = 0
        for w, grp in zip(top["chunks"], groups):
            assert len(w["tokens"]) == len(grp) > 0
            assert w["logprob"] == float(np.sum(np.asarray([t["logprob"] for t in w["tokens"]], np.float64)))
            for t, i in zip(w["tokens"], grp):
                assert t["id"] == int(toks[i]) and t["logprob"] == float(lp[i]) and t["text"] == token_text(pipe.vocab, toks[i])
                assert [(a["id"], a["logprob"]) for a in t["top_logprobs"]] == [(int(a), float(b)) for a, b in zip(tid[i], tlp[i]) if a >= 0]
                assert all(a["text"] == token_text(pipe.vocab, a["id"]) for a in t["top_logprobs"])
                n_alt += len(t["top_logprobs"])
        assert n_alt == k * sum(len(grp) for grp in groups)      # V finite logits at every step: no rank is empty
        if call == "fallback":
            assert any(r["temperature_index"] > 0 for r in pipe.stats["fallback"])
        with pytest.raises(ValueError, match="num_beams"):
            pipe(x, generate_kwargs=dict(gk, num_beams=5), top_logprobs=k)
        again = pipe(x, generate_kwargs=dict(gk))                # ... and the refusal left nothing behind
        assert again == scored
    finally:
        pipe.engine.close()
