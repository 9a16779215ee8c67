"""Host side of top_logprobs: segment slicing, generate's argument checks (a refused call touches no engine state), the gather
record at its three widths, the pipeline's per-word "tokens" against hand-built groups, and the pipeline's refusals.  Host-only:
no GPU."""
import numpy as np
import pytest

from crisperwhisper_amd import _native, collate, dist, generation, synthetic as syn
from crisperwhisper_amd.pipeline import CrisperWhisperPipeline, scored_words, token_text
from tests import helpers as Hh
from tests.test_token_logprobs_host import _window


def test_exported_symbols():
    for name in ("cw_set_top_logprobs", "cw_get_top_logprobs", "cw_get_transcribe_top_logprobs", "cw_test_sample_top_logprobs"):
        assert name in _native.exported_symbols()
    assert _native.load().cw_abi_version() == 1
    assert generation.TOP_LOGPROBS_MAX == 8


def test_split_segments_cuts_the_alternatives_like_the_timestamps():
    tb, k = 1000, 3
    seq = np.array([tb, 5, 6, tb + 10, tb + 10, 7, tb + 20, tb + 20, 8], np.int64)
    n_prompt = 3
    n = n_prompt + len(seq)
    ts = np.arange(n, dtype=np.float32)
    lp = -np.arange(n, dtype=np.float32)
    tid = (np.arange(n * k).reshape(n, k) * 7 % 1000).astype(np.int32)
    tlp = -(np.arange(n * k).reshape(n, k) / 8).astype(np.float32)
    segs, adv = generation.split_segments(seq, ts, 0.0, tb, 3000, n_prompt, lp, (tid, tlp))
    plain, adv2 = generation.split_segments(seq, ts, 0.0, tb, 3000, n_prompt, lp)
    assert adv == adv2 and len(segs) == len(plain) == 2
    for s, p in zip(segs, plain):
        assert p.top_ids is None and p.top_logprobs is None
        assert np.array_equal(s.tokens, p.tokens) and s.idxs == p.idxs and np.array_equal(s.token_logprobs, p.token_logprobs)
        a, b = s.idxs
        assert s.top_ids.dtype == np.int32 and s.top_logprobs.dtype == np.float32
        assert s.top_ids.shape == s.top_logprobs.shape == (len(s.tokens), k)
        assert np.array_equal(s.top_ids, tid[a:b]) and np.array_equal(s.top_logprobs, tlp[a:b])
    # the window without a closing pair: one segment over the whole row
    seq = np.array([tb, 5, 6, 7], np.int64)
    segs, _ = generation.split_segments(seq, ts, 0.0, tb, 3000, n_prompt, lp, (tid, tlp))
    assert len(segs) == 1 and np.array_equal(segs[0].top_ids, tid[3:7]) and np.array_equal(segs[0].top_logprobs, tlp[3:7])
    assert generation.Segment(seq, ts[:4], (0, 4)).top_ids is None


class _Recorder:
    """An engine that records every call that would change its state."""

    def __init__(self, spec, with_top=True):
        self.spec, self.max_batch, self.calls = spec, 64, []
        if with_top:
            self.set_top_logprobs = lambda k: self.calls.append(("set_top_logprobs", k))

    def set_thresholds(self, *a):
        self.calls.append(("set_thresholds",) + a)

    def set_token_logprobs(self, on):
        self.calls.append(("set_token_logprobs", on))

    def set_sampling(self, *a):
        self.calls.append(("set_sampling",) + a)

    def __getattr__(self, name):                       # anything else: absent (hasattr), and calling it would fail
        raise AttributeError(f"engine.{name} reached by a call that must be refused")


@pytest.mark.parametrize("kw, match", [
    (dict(top_logprobs=3), "return_token_logprobs"),
    (dict(top_logprobs=9, return_token_logprobs=True), "0 .. 8"),
    (dict(top_logprobs=-1, return_token_logprobs=True), "0 .. 8"),
    (dict(top_logprobs=2.5, return_token_logprobs=True), "0 .. 8"),
    (dict(top_logprobs=True, return_token_logprobs=True), "0 .. 8"),
    (dict(top_logprobs=5, return_token_logprobs=True, num_beams=5), "num_beams=1"),
])
def test_generate_refusals_leave_no_engine_state_behind(kw, match):
    g, v, W, spec = Hh.tiny_setup()
    eng = _Recorder(spec)
    with pytest.raises(ValueError, match=match):
        generation.generate(eng, 1, [3000], language="<|en|>", task="transcribe", **kw)
    assert eng.calls == []
    eng = _Recorder(spec, with_top=False)
    with pytest.raises(ValueError):
        generation.generate(eng, 1, [3000], language="<|en|>", task="transcribe", return_token_logprobs=True, top_logprobs=2)
    assert eng.calls == []


def test_record_round_trip_at_the_three_widths():
    toks, ts, stride = np.array([1, 2, 300]), np.array([0.5, 1.25, 2.0], np.float32), (30.0, 5.0, 0.0)
    lp = np.array([-0.25, 0.0, -17.5], np.float32)
    plain = dist.pack_record(7, toks, ts, stride)
    want = np.zeros(dist.REC_WORDS, np.int32)           # the default record, byte for byte
    want[0:3] = (7, 3, 3)
    want[3:6] = np.asarray(stride, np.float32).view(np.int32)
    want[6:9] = toks
    want[6 + dist.REC_TOKENS:9 + dist.REC_TOKENS] = ts.view(np.int32)
    assert plain.tobytes() == want.tobytes() and len(dist.unpack_record(plain)) == 4
    scored = dist.pack_record(7, toks, ts, stride, lp)
    want2 = np.zeros(dist.REC_WORDS_SCORED, np.int32)   # the scored record, byte for byte
    want2[:dist.REC_WORDS] = want
    want2[dist.REC_WORDS:dist.REC_WORDS + 3] = lp.view(np.int32)
    assert dist.REC_WORDS_SCORED == dist.REC_WORDS + dist.REC_TOKENS
    assert scored.tobytes() == want2.tobytes() and len(dist.unpack_record(scored)) == 5
    for k in (1, 5, 8):
        tid = np.arange(3 * k, dtype=np.int32).reshape(3, k) - 1                 # a -1 among them
        tlp = -(np.arange(3 * k, dtype=np.float32).reshape(3, k) / 4)
        tlp[0, 0] = np.nan
        wide = dist.pack_record(7, toks, ts, stride, lp, (tid, tlp))
        assert wide.shape == (dist.REC_WORDS_SCORED + 2 * k * dist.REC_TOKENS,) == (dist.rec_words_top(k),)
        assert wide.dtype == np.int32 and wide[:dist.REC_WORDS_SCORED].tobytes() == scored.tobytes()
        idx, t2, ts2, st2, lp2, tid2, tlp2 = dist.unpack_record(wide)
        assert idx == 7 and t2.tolist() == toks.tolist() and ts2.tobytes() == ts.tobytes() and st2 == stride
        assert lp2.tobytes() == lp.tobytes()
        assert tid2.dtype == np.int32 and tid2.shape == (3, k) and tid2.tobytes() == tid.tobytes()
        assert tlp2.dtype == np.float32 and tlp2.shape == (3, k) and tlp2.tobytes() == tlp.tobytes()
        # an empty shard sends the width the other ranks send
        assert dist.Shard().all_gather_records(np.zeros((0, dist.rec_words_top(k)), np.int32), 2).shape == (0, dist.rec_words_top(k))
    z = np.zeros(0, np.float32)
    empty = dist.unpack_record(dist.pack_record(3, np.zeros(0, np.int64), z, stride, z, (np.zeros((0, 5), np.int32), np.zeros((0, 5), np.float32))))
    assert len(empty) == 7 and empty[5].shape == (0, 5) and empty[6].shape == (0, 5)
    with pytest.raises(ValueError):
        dist.pack_record(7, toks, ts, stride, None, (np.zeros((3, 2), np.int32), np.zeros((3, 2), np.float32)))   # no scores
    with pytest.raises(ValueError):
        dist.pack_record(7, toks, ts, stride, lp, (np.zeros((2, 2), np.int32), np.zeros((2, 2), np.float32)))     # a row short
    with pytest.raises(ValueError):
        dist.unpack_record(np.zeros(dist.REC_WORDS_SCORED + 5, np.int32))


def test_word_tokens_over_hand_built_groups():
    g, v = syn.tiny_geometry()
    vocab = collate.Vocabulary.from_synthetic(v)
    k = 3
    a_tok, a_ts, a_lp = _window(v, ["ab", "cd", "ef", "gh"], 0.0, 29.0, 0)
    b_tok, b_ts, b_lp = _window(v, ["ef", "gh", "ij", "kl"], 1.0, 20.0, len(a_tok))
    outputs = [{"tokens": a_tok, "token_timestamps": a_ts, "stride": (30.0, 0.0, 5.0)},
               {"tokens": b_tok, "token_timestamps": b_ts, "stride": (30.0, 5.0, 0.0)}]

    def alts(tok, lp, base):
        """[n][k]: the token itself, a neighbour byte, and nothing (-1 / NaN) at every other position"""
        n = len(tok)
        tid = np.stack([tok, (tok + 1) % 256, np.where(np.arange(n) % 2 == 0, -1, ord("z"))], axis=1).astype(np.int32)
        tlp = np.stack([lp, lp - 1, np.where(np.arange(n) % 2 == 0, np.nan, lp - 2 - base)], axis=1).astype(np.float32)
        return tid, tlp

    top = [alts(a_tok, a_lp, 0), alts(b_tok, b_lp, 1)]
    text0, words0 = scored_words(vocab, [dict(o) for o in outputs], [a_lp, b_lp])
    text, words = scored_words(vocab, [dict(o) for o in outputs], [a_lp, b_lp], token_top=top)
    _, _, groups = collate.decode_asr(vocab, [dict(o) for o in outputs], return_timestamps="word", return_token_groups=True)
    assert text == text0 and all("tokens" not in w for w in words0)
    assert [{x: w[x] for x in ("text", "timestamp", "logprob")} for w in words] == words0      # nothing else changes
    flat_tok = np.concatenate([a_tok, b_tok]); flat_lp = np.concatenate([a_lp, b_lp])
    flat_id = np.concatenate([top[0][0], top[1][0]]); flat_tl = np.concatenate([top[0][1], top[1][1]])
    assert [w["text"] for w in words] == [" ab", " cd", " ef", " gh", " ij", " kl"]
    for w, grp in zip(words, groups):
        assert [t["id"] for t in w["tokens"]] == [int(flat_tok[i]) for i in grp]
        assert "".join(t["text"] for t in w["tokens"]) == w["text"]
        for t, i in zip(w["tokens"], grp):
            assert t["logprob"] == float(flat_lp[i]) and set(t) == {"id", "text", "logprob", "top_logprobs"}
            want = [(int(a), float(b)) for a, b in zip(flat_id[i], flat_tl[i]) if a >= 0]
            assert len(want) == (2 if i % len(a_tok) % 2 == 0 and i < len(a_tok) or (i >= len(a_tok) and (i - len(a_tok)) % 2 == 0) else 3)
            assert [(x["id"], x["logprob"]) for x in t["top_logprobs"]] == want
            assert all(x["text"] == token_text(vocab, x["id"]) and set(x) == {"id", "text", "logprob"} for x in t["top_logprobs"])
            assert t["top_logprobs"][0]["logprob"] == t["logprob"]               # the token itself leads its own list here
    with pytest.raises(ValueError):
        scored_words(vocab, [dict(o) for o in outputs], [a_lp, b_lp], token_top=[top[0], (top[1][0][:-1], top[1][1][:-1])])


def test_token_text_decodes_bytes_with_replacement():
    g, v = syn.tiny_geometry()
    vocab = collate.Vocabulary.from_synthetic(v)
    assert token_text(vocab, ord("a")) == "a"
    assert token_text(vocab, 0xE9) == b"\xe9".decode("utf-8", errors="replace") == "�"     # half a character
    assert token_text(vocab, v.eos) == vocab.specials[v.eos]
    assert token_text(vocab, v.timestamp_begin + 50) == "<|1.00|>"


def _bare_pipeline(spec, **attrs):
    p = object.__new__(CrisperWhisperPipeline)
    p.bundle = type("B", (), {"spec": spec})()
    p.sampling_seed = None
    p.return_timestamps = "word"
    p.return_scores = False
    p.top_logprobs = 0
    p.default_num_beams = 5
    for a, x in attrs.items():
        setattr(p, a, x)
    return p


def test_pipeline_refusals():
    """Every refusal comes before the audio is loaded: the input here is no audio at all (loading it raises TypeError)."""
    g, v, W, spec = Hh.tiny_setup()
    greedy = {"num_beams": 1}
    p = _bare_pipeline(spec)
    with pytest.raises(ValueError, match="return_scores"):
        p._run_one(12345, top_logprobs=3, generate_kwargs=greedy)                          # no return_scores
    with pytest.raises(ValueError, match="word"):
        p._run_one(12345, top_logprobs=3, return_scores=True, return_timestamps=True, generate_kwargs=greedy)   # segment mode
    with pytest.raises(ValueError, match="num_beams"):
        p._run_one(12345, top_logprobs=3, return_scores=True, generate_kwargs={"num_beams": 5})
    with pytest.raises(ValueError, match="num_beams"):
        p._run_one(12345, top_logprobs=3, return_scores=True)                              # the default beam width
    with pytest.raises(ValueError, match="0 .. 8"):
        p._run_one(12345, top_logprobs=9, return_scores=True, generate_kwargs=greedy)
    p = _bare_pipeline(spec, top_logprobs=4, return_scores=True)                           # the constructor's values
    with pytest.raises(ValueError, match="num_beams"):
        p._run_one(12345)
    with pytest.raises(TypeError):
        p._run_one(12345, generate_kwargs=greedy)                                          # accepted: only now is the input loaded
    p = _bare_pipeline(spec, top_logprobs=0, return_scores=True)
    with pytest.raises(TypeError):
        p._run_one(12345, generate_kwargs={"num_beams": 5})                                # beams without alternatives: as before
