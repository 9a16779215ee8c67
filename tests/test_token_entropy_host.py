"""Host side of token entropy: the C ABI surface, segment slicing, generate's and the pipeline's refusals (a refused call touches no
engine state and loads no audio), the gather record's entropy tail, and the per-word aggregation over hand-built groups with a
seam-dropped token and a NaN.  Host-only: no GPU."""
import copy

import numpy as np
import pytest

from crisperwhisper_amd import _native, collate, dist, generation, synthetic as syn
from crisperwhisper_amd.pipeline import add_token_entropy, scored_words
from tests import helpers as Hh
from tests.test_token_logprobs_host import _window
from tests.test_top_logprobs_host import _Recorder, _bare_pipeline


def test_exported_symbols():
    for name in ("cw_set_token_entropy", "cw_get_token_entropy", "cw_get_transcribe_token_entropy", "cw_test_sample_entropy",
                 "cw_set_score_entropy", "cw_get_score_entropy", "cw_test_score_head_entropy", "cw_test_score_rows_entropy",
                 "cw_time_score_head_entropy"):
        assert name in _native.exported_symbols()
    assert _native.load().cw_abi_version() == 1


def test_split_segments_cuts_the_entropy_like_the_timestamps():
    tb = 1000
    seq = np.array([tb, 5, 6, tb + 10, tb + 10, 7, tb + 20, tb + 20, 8], np.int64)
    n_prompt = 3
    n = n_prompt + len(seq)
    ts = np.arange(n, dtype=np.float32)
    lp = -np.arange(n, dtype=np.float32)
    en = (np.arange(n, dtype=np.float32) / 4)
    segs, adv = generation.split_segments(seq, ts, 0.0, tb, 3000, n_prompt, lp, token_ent=en)
    plain, adv2 = generation.split_segments(seq, ts, 0.0, tb, 3000, n_prompt, lp)
    assert adv == adv2 and len(segs) == len(plain) == 2
    for s, p in zip(segs, plain):
        assert p.token_entropy is None and np.array_equal(s.tokens, p.tokens) and s.idxs == p.idxs
        assert np.array_equal(s.token_logprobs, p.token_logprobs)
        a, b = s.idxs
        assert s.token_entropy.dtype == np.float32 and np.array_equal(s.token_entropy, en[a:b])
    segs, _ = generation.split_segments(np.array([tb, 5, 6, 7], np.int64), ts, 0.0, tb, 3000, n_prompt, lp, token_ent=en)
    assert len(segs) == 1 and np.array_equal(segs[0].token_entropy, en[3:7])


@pytest.mark.parametrize("kw, match", [
    (dict(return_token_entropy=True), "return_token_logprobs"),
    (dict(return_token_entropy=True, return_token_logprobs=True, num_beams=5), "num_beams=1"),
])
def test_generate_refusals_leave_no_engine_state_behind(kw, match):
    g, v, W, spec = Hh.tiny_setup()
    eng = _Recorder(spec)
    eng.set_token_entropy = lambda on: eng.calls.append(("set_token_entropy", on))
    with pytest.raises(ValueError, match=match):
        generation.generate(eng, 1, [3000], language="<|en|>", task="transcribe", **kw)
    assert eng.calls == []
    eng = _Recorder(spec)                               # an engine without the switch
    with pytest.raises(ValueError, match="cw_set_token_entropy"):
        generation.generate(eng, 1, [3000], language="<|en|>", task="transcribe", return_token_logprobs=True, return_token_entropy=True)
    assert eng.calls == []


def test_pipeline_refusals():
    """Every refusal comes before the audio is loaded: the input here is no audio at all (loading it raises TypeError)."""
    g, v, W, spec = Hh.tiny_setup()
    greedy = {"num_beams": 1}
    p = _bare_pipeline(spec)
    with pytest.raises(ValueError, match="return_scores"):
        p._run_one(12345, return_entropy=True, generate_kwargs=greedy)                          # no return_scores
    with pytest.raises(ValueError, match="word"):
        p._run_one(12345, return_entropy=True, return_scores=True, return_timestamps=True, generate_kwargs=greedy)
    with pytest.raises(ValueError, match="num_beams"):
        p._run_one(12345, return_entropy=True, return_scores=True, generate_kwargs={"num_beams": 5})
    with pytest.raises(ValueError, match="num_beams"):
        p._run_one(12345, return_entropy=True, return_scores=True)                              # the pipeline's default beam width
    with pytest.raises(ValueError, match="generate_kwargs"):
        p._run_one(12345, return_scores=True, generate_kwargs={"num_beams": 1, "return_entropy": True})   # not a generate_kwargs key
    p = _bare_pipeline(spec, return_entropy=True, return_scores=True)                           # the constructor's values
    with pytest.raises(ValueError, match="num_beams"):
        p._run_one(12345)
    with pytest.raises(TypeError):
        p._run_one(12345, generate_kwargs=greedy)                                               # accepted: only now is the input loaded


def test_record_tail_round_trip():
    toks, ts, stride = np.array([1, 2, 300]), np.array([0.5, 1.25, 2.0], np.float32), (30.0, 5.0, 0.0)
    lp = np.array([-0.25, 0.0, -17.5], np.float32)
    en = np.array([0.0, np.nan, 5.25], np.float32)
    for rec in (dist.pack_record(7, toks, ts, stride, lp),
                dist.pack_record(7, toks, ts, stride, lp, (np.zeros((3, 2), np.int32), np.zeros((3, 2), np.float32))),
                dist.append_alignment(dist.pack_record(7, toks, ts, stride, lp), en, en)):
        wide = dist.append_entropy(rec, en)
        assert wide.dtype == np.int32 and len(wide) == len(rec) + dist.REC_ENTROPY_WORDS
        back, en2 = dist.split_entropy(wide)
        assert back.tobytes() == rec.tobytes() and en2.tobytes() == en.tobytes()
    with pytest.raises(ValueError):
        dist.append_entropy(dist.pack_record(7, toks, ts, stride, lp), en[:2])
    with pytest.raises(ValueError):
        dist.split_entropy(np.zeros(dist.REC_WORDS, np.int32))


def test_word_entropy_over_hand_built_groups():
    g, v = syn.tiny_geometry()
    vocab = collate.Vocabulary.from_synthetic(v)
    a_tok, a_ts, a_lp = _window(v, ["ab", "cd", "ef", "gh"], 0.0, 29.0, 0)
    b_tok, b_ts, b_lp = _window(v, ["ef", "gh", "ij", "kl"], 1.0, 20.0, len(a_tok))
    outputs = [{"tokens": a_tok, "token_timestamps": a_ts, "stride": (30.0, 0.0, 5.0)},
               {"tokens": b_tok, "token_timestamps": b_ts, "stride": (30.0, 5.0, 0.0)}]
    rng = np.random.default_rng(0)
    a_en = rng.uniform(0, 5, len(a_tok)).astype(np.float32)
    b_en = rng.uniform(0, 5, len(b_tok)).astype(np.float32)
    text, words, groups = scored_words(vocab, [dict(o) for o in outputs], [a_lp, b_lp], return_groups=True)
    before = copy.deepcopy(words)
    flat = np.concatenate([a_en, b_en]).astype(np.float64)
    used = sorted(i for grp in groups for i in grp)
    dropped = sorted(set(range(len(flat))) - set(used))
    assert dropped, "the seam merge drops the overlap's tokens of one window: they belong to no group"
    nan_at = int(groups[1][0])                                        # one NaN inside the second word
    en = [a_en.copy(), b_en.copy()]
    (en[0] if nan_at < len(a_tok) else en[1])[nan_at % len(a_tok) if nan_at >= len(a_tok) else nan_at] = np.nan
    flat = np.concatenate(en).astype(np.float64)
    add_token_entropy(words, groups, en)
    assert [w["text"] for w in words] == [" ab", " cd", " ef", " gh", " ij", " kl"]
    for w, w0, grp in zip(words, before, groups):
        assert {k: x for k, x in w.items() if k not in ("entropy", "entropy_max")} == w0        # nothing else changes
        h = flat[np.asarray(grp, np.int64)]
        if np.isnan(h).any():
            assert np.isnan(w["entropy"]) and np.isnan(w["entropy_max"])
        else:
            assert w["entropy"] == float(np.mean(h)) and w["entropy_max"] == float(np.max(h)) and isinstance(w["entropy"], float)
    assert sum(np.isnan(w["entropy"]) for w in words) == 1
    # a token the seam merge dropped counts in no word: moving its value moves nothing
    words2 = copy.deepcopy(before)
    en2 = [x.copy() for x in en]
    for i in dropped:
        (en2[0] if i < len(a_tok) else en2[1])[i if i < len(a_tok) else i - len(a_tok)] = 99.0
    add_token_entropy(words2, groups, en2)
    for w, w2 in zip(words, words2):
        assert (w["entropy"] == w2["entropy"] or (np.isnan(w["entropy"]) and np.isnan(w2["entropy"])))
    # "tokens" entries (top_logprobs) gain their own value
    k = 2
    top = [(np.stack([t, t], 1).astype(np.int32), np.stack([l, l - 1], 1).astype(np.float32)) for t, l in ((a_tok, a_lp), (b_tok, b_lp))]
    _, words3, groups3 = scored_words(vocab, [dict(o) for o in outputs], [a_lp, b_lp], token_top=top, return_groups=True)
    add_token_entropy(words3, groups3, en)
    for w, grp in zip(words3, groups3):
        got = [t["entropy"] for t in w["tokens"]]
        want = [float(flat[i]) for i in grp]
        assert all((a == b) or (np.isnan(a) and np.isnan(b)) for a, b in zip(got, want)) and len(got) == len(want)


def test_return_entropy_false_is_the_call_without_it():
    """With engine doubles (tests/language_doubles.py: three strided windows with seam overlaps): return_entropy=False, the
    constructor's False and the argument left out give the same result byte for byte, and the engine is never asked for the switch
    or for a getter of the entropy."""
    import pickle
    from tests import language_doubles as LD
    g, v, W, spec = Hh.tiny_setup()

    class Eng(LD.LangScriptedEngine):
        touched = []

        def set_token_entropy(self, on):
            if on:
                self.touched.append("set_token_entropy(True)")

        def token_entropy(self, nb):
            self.touched.append("token_entropy")

        def transcribe_token_entropy(self, lens):
            self.touched.append("transcribe_token_entropy")

    def run(ctor=None, **call):
        p = LD.make_pipe(spec, v, Eng(spec, v, [0, 1, 2]), batch_size=2)
        if ctor is not None:
            p.return_entropy = ctor
        return p(LD.PCM, return_scores=True, top_logprobs=2, generate_kwargs={"num_beams": 1}, **call)

    base = run()
    assert len(base["chunks"]) > 3 and all("entropy" not in w and "entropy_max" not in w for w in base["chunks"])
    assert all("entropy" not in t for w in base["chunks"] for t in w["tokens"])
    for other in (run(return_entropy=False), run(ctor=False), run(ctor=True, return_entropy=False)):
        assert pickle.dumps(other) == pickle.dumps(base)
    assert Eng.touched == []
    # ... and with it on, the double is asked, and only the new keys differ
    class On(Eng):
        def transcribe_token_entropy(self, lens):
            return [(-self.script[k][2] / 100).astype(np.float32) for k in self.batch]

    p = LD.make_pipe(spec, v, On(spec, v, [0, 1, 2]), batch_size=2)
    on = p(LD.PCM, return_scores=True, top_logprobs=2, return_entropy=True, generate_kwargs={"num_beams": 1})
    strip = lambda w: {k: ([{kk: x for kk, x in t.items() if kk != "entropy"} for t in val] if k == "tokens" else val)
                       for k, val in w.items() if k not in ("entropy", "entropy_max")}
    assert on["text"] == base["text"] and pickle.dumps([strip(w) for w in on["chunks"]]) == pickle.dumps(base["chunks"])
    for w in on["chunks"]:                              # the double's value names its token: entropy = -logprob / 100
        want = [np.float64(np.float32(-np.float32(t["logprob"]) / 100)) for t in w["tokens"]]
        assert [t["entropy"] for t in w["tokens"]] == [float(x) for x in want]
        assert w["entropy"] == float(np.mean(want)) and w["entropy_max"] == float(np.max(want))
