"""Host logic of transcript scoring (generation.score, CrisperWhisperPipeline.score, align(return_scores=True)): exported symbols,
argument checks that come before any device work, the grouping of ragged candidate lists into engine calls, and the collator's
word token groups against transformers' own word combiner (tests/golden/e2e_score_golden.json).  No GPU: a stand-in engine
records the calls."""
import ctypes

import numpy as np
import pytest

from crisperwhisper_amd import _native, collate, generation, synthetic as syn
from crisperwhisper_amd.pipeline import CrisperWhisperPipeline
from tests import helpers as Hh

GOLD = Hh.gold_json("e2e_score_golden.json")


@pytest.fixture(scope="module")
def tiny():
    return Hh.tiny_setup()


class FakeEngine:
    def __init__(self, spec, max_batch=4):
        self.spec, self.max_batch, self.calls, self.mels = spec, max_batch, [], []

    def mel(self, clips):
        self.mels.append([len(c) for c in clips])
        return None, np.asarray([min(3000, len(c) // 160) for c in clips])

    def score_tokens(self, rows, n_init, rows_per_item=1):
        self.calls.append(("score", [np.asarray(r).copy() for r in rows], n_init, rows_per_item))
        # token k of a row scores -(k + 1) / 8 - its id / 1024: every entry tells its row and place
        lp = [-(np.arange(len(r) - n_init) + 1) / 8.0 - np.asarray(r[n_init:]) / 1024.0 for r in rows]
        return ([a.astype(np.float32) for a in lp], [np.asarray(r[n_init:], np.int64) for r in rows],
                [a.astype(np.float32) / 2 for a in lp])

    def align_score_tokens(self, num_frames, ids, n_init):
        lp, ti, tl = self.score_tokens(ids, n_init)
        self.calls[-1] = ("align_score",) + self.calls[-1][1:]
        return [np.arange(len(r), dtype=np.float32) * 0.02 for r in ids], lp, ti, tl

    def align_tokens(self, num_frames, ids, n_init):
        self.calls.append(("align", [np.asarray(r).copy() for r in ids], n_init, 1))
        return [np.arange(len(r), dtype=np.float32) * 0.02 for r in ids]


def _pipe(spec, v, eng=None):
    p = object.__new__(CrisperWhisperPipeline)
    p.bundle = type("B", (), {"spec": spec})()
    p.vocab = collate.Vocabulary.from_synthetic(v)
    p.tokenizer = p.vocab
    p.sampling_rate = 16000
    p.engine = eng
    p.engines = [eng]
    return p


def test_exported_symbols_and_prototypes():
    lib = _native.load()
    for name in ("cw_score_tokens", "cw_align_score_tokens", "cw_score_prefill_runs", "cw_test_score_head",
                 "cw_collate_get_token_groups", "cw_collate_token_groups_total"):
        assert name in _native.exported_symbols()
        assert getattr(lib, name) is not None
    assert len(lib.cw_score_tokens.argtypes) == 10 and lib.cw_score_tokens.restype is ctypes.c_int32
    assert len(lib.cw_align_score_tokens.argtypes) == 11
    assert len(lib.cw_test_score_head.argtypes) == 12
    assert lib.cw_align_tokens.argtypes is not None and len(lib.cw_align_tokens.argtypes) == 8      # signature kept
    header = open(Hh.ROOT + "/include/crisperwhisper.h").read()
    for name in ("cw_score_tokens", "cw_align_score_tokens", "cw_score_prefill_runs", "cw_test_score_head", "cw_time_score_head",
                 "cw_collate_get_token_groups"):
        assert name + "(" in header


def test_plan_score_calls_groups_and_splits():
    plan = generation.plan_score_calls([1, 4, 1, 2, 4, 1], 8)
    assert plan == [(1, [(0, 0), (2, 0), (5, 0)]), (2, [(3, 0)]), (4, [(1, 0), (4, 0)])]
    # a group that would exceed max_batch rows is split; one item with more candidates than rows is split across calls
    plan = generation.plan_score_calls([3, 3, 3, 11], 8)
    assert plan == [(3, [(0, 0), (1, 0)]), (3, [(2, 0), (3, 8)]), (8, [(3, 0)])]
    for ks, mb in [([1, 4, 1, 2, 4, 1], 8), ([3, 3, 3, 11], 8), ([5], 2), ([7, 1, 9, 2, 2], 4)]:
        seen = []
        for rpi, members in generation.plan_score_calls(ks, mb):
            assert 1 <= rpi <= mb and rpi * len(members) <= mb
            seen += [(b, c0 + j) for b, c0 in members for j in range(rpi)]
        assert sorted(seen) == [(b, k) for b, n in enumerate(ks) for k in range(n)] and len(set(seen)) == len(seen)
    with pytest.raises(ValueError, match="no candidates"):
        generation.plan_score_calls([1, 0], 4)


def test_generation_score_rows_and_results(tiny):
    g, v, W, spec = tiny
    eng = FakeEngine(spec, max_batch=4)
    loads = []
    out = generation.score(eng, 2, [[[5, 6, 7], [8]], [[9, 10]]], language="<|en|>", task="transcribe", load_items=loads.append)
    init = [v.sot, v.lang_id("en"), v.transcribe]
    (_, rows1, n1, rpi1), (_, rows2, n2, rpi2) = eng.calls
    assert (n1, rpi1, n2, rpi2) == (3, 1, 3, 2)
    assert [r.tolist() for r in rows1] == [init + [9, 10, v.eos]]
    assert [r.tolist() for r in rows2] == [init + [5, 6, 7, v.eos], init + [8, v.eos]]
    assert loads == [[1], [0], [0, 1]]                     # item 1 alone, then item 0, then the caller's state again
    assert out[0][1]["ids"].tolist() == [8] and len(out[0][1]["token_logprobs"]) == 2
    assert np.allclose(out[1][0]["token_logprobs"], [-1 / 8 - 9 / 1024, -2 / 8 - 10 / 1024, -3 / 8 - v.eos / 1024])
    # one candidate count over items 0 .. n-1 needs no reload
    eng = FakeEngine(spec, max_batch=4)
    generation.score(eng, 2, [[[5]], [[6, 7]]], language="<|en|>", task="transcribe")
    assert len(eng.calls) == 1 and eng.calls[0][3] == 1
    with pytest.raises(ValueError, match="load_items"):
        generation.score(FakeEngine(spec, 4), 2, [[[5], [6]], [[7]]], language="<|en|>", task="transcribe")


def test_generation_score_refusals(tiny):
    g, v, W, spec = tiny
    eng = FakeEngine(spec, max_batch=2)
    kw = dict(language="<|en|>", task="transcribe")
    with pytest.raises(ValueError, match="empty candidate list"):
        generation.score(eng, 1, [[]], **kw)
    with pytest.raises(ValueError, match="candidate lists for"):
        generation.score(eng, 2, [[[1]]], **kw)
    with pytest.raises(ValueError, match="exceed the engine"):
        generation.score(eng, 3, [[[1]]] * 3, **kw)
    with pytest.raises(ValueError, match="special"):
        generation.score(eng, 1, [[[1, v.eos]]], **kw)
    with pytest.raises(ValueError, match="max_target_positions"):
        generation.score(eng, 1, [[[1] * spec.max_target_positions]], **kw)
    with pytest.raises(ValueError):
        generation.score(eng, 1, [[[1]]], language="<|xx|>", task="transcribe")
    assert eng.calls == [] and eng.mels == []


def test_pipeline_score_forms_and_arithmetic(tiny):
    g, v, W, spec = tiny
    eng = FakeEngine(spec, max_batch=4)
    p = _pipe(spec, v, eng)
    x = np.zeros(16000, np.float32)
    text = [ord(c) for c in " ab cd"]
    one = p.score(x, text, language="<|en|>", task="transcribe")
    assert isinstance(one, dict) and one["text"] == " ab cd"
    assert [c["text"] for c in one["chunks"]] == [" ab", " cd"]
    lps = [t["logprob"] for t in one["tokens"]]
    assert len(lps) == len(text) + 1 and one["tokens"][-1]["id"] == v.eos
    assert one["logprob"] == pytest.approx(sum(lps)) and one["avg_logprob"] == pytest.approx(sum(lps) / (len(text) + 1))
    assert one["chunks"][0]["logprob"] == pytest.approx(sum(lps[:3])) and one["chunks"][1]["logprob"] == pytest.approx(sum(lps[3:6]))
    many = p.score([x, x], [[text, np.asarray(text[:3])], tuple(text)], language="<|en|>", task="transcribe")
    assert isinstance(many[0], list) and len(many[0]) == 2 and isinstance(many[1], dict)
    assert many[0][1]["text"] == " ab" and many[1]["text"] == " ab cd"
    assert one["logprob"] == pytest.approx(many[1]["logprob"])


def test_pipeline_score_refusals_before_audio(tiny):
    g, v, W, spec = tiny
    eng = FakeEngine(spec, max_batch=4)
    p = _pipe(spec, v, eng)
    x = np.zeros(16000, np.float32)
    with pytest.raises(ValueError, match="empty candidate list"):
        p.score(x, [])
    with pytest.raises(ValueError, match="mixes"):
        p.score(x, [1, [2, 3]])
    with pytest.raises(ValueError, match="tokenizer with `encode`"):
        p.score(x, "some text")
    with pytest.raises(ValueError, match="prompt_ids"):
        p.score(x, [1], prompt_ids=[1])
    with pytest.raises(TypeError):
        p.score(x, [1], num_beams=2)
    with pytest.raises(ValueError, match="2 inputs need"):
        p.score([x, x], [[1]])
    with pytest.raises(ValueError, match="special"):
        p.score(x, [[1], [v.sot]])
    with pytest.raises(ValueError, match="at most 30 s"):
        p.score(np.zeros(16000 * 31, np.float32), [1], language="<|en|>")
    assert eng.calls == [] and eng.mels == []


def test_pipeline_align_return_scores(tiny):
    g, v, W, spec = tiny
    eng = FakeEngine(spec, max_batch=4)
    p = _pipe(spec, v, eng)
    x = np.zeros(16000, np.float32)
    text = [ord(c) for c in " ab cd"]
    plain = p.align(x, text, language="<|en|>", task="transcribe")
    assert eng.calls[-1][0] == "align" and set(plain) == {"text", "chunks"} and set(plain["chunks"][0]) == {"text", "timestamp"}
    scored = p.align(x, text, language="<|en|>", task="transcribe", return_scores=True)
    assert eng.calls[-1][0] == "align_score"
    assert [(c["text"], c["timestamp"]) for c in scored["chunks"]] == [(c["text"], c["timestamp"]) for c in plain["chunks"]]
    s = p.score(x, text, language="<|en|>", task="transcribe")
    assert [c["logprob"] for c in scored["chunks"]] == [c["logprob"] for c in s["chunks"]]
    assert scored["logprob"] == s["logprob"] and scored["avg_logprob"] == s["avg_logprob"]


def test_collator_token_groups_match_transformers(tiny):
    g, v, W, spec = tiny
    vocab = collate.Vocabulary.from_synthetic(v)
    for c in GOLD["cases"]:
        ids = c["ids"]
        text, words, groups = collate.decode_asr(vocab, [{"tokens": ids, "token_timestamps": np.zeros(len(ids), np.float32)}],
                                                 return_timestamps="word", return_token_groups=True)
        assert [w["text"] for w in words] == c["chunks"], c["name"]
        assert groups == c["word_groups"], c["name"]
        assert sorted(i for grp in groups for i in grp) == list(range(len(ids)))          # every token exactly once
        text2, words2 = collate.decode_asr(vocab, [{"tokens": ids, "token_timestamps": np.zeros(len(ids), np.float32)}],
                                           return_timestamps="word")
        assert (text2, words2) == (text, words)


def test_collator_token_groups_skip_timestamp_tokens_and_count_across_feeds(tiny):
    g, v, W, spec = tiny
    vocab = collate.Vocabulary.from_synthetic(v)
    tb = v.timestamp_begin
    ids = [tb] + [ord(c) for c in " ab"] + [tb + 10, tb + 10] + [ord(c) for c in " c"] + [tb + 20]
    _, words, groups = collate.decode_asr(vocab, [{"tokens": ids, "token_timestamps": np.zeros(len(ids), np.float32)}],
                                          return_timestamps="word", return_token_groups=True)
    assert [w["text"] for w in words] == [" ab", " c"] and groups == [[1, 2, 3], [6, 7]]
    two = [{"tokens": [ord(c) for c in " ab"], "token_timestamps": np.zeros(3, np.float32)},
           {"tokens": [ord(c) for c in " cd"], "token_timestamps": np.zeros(3, np.float32)}]
    _, words, groups = collate.decode_asr(vocab, two, return_timestamps="word", return_token_groups=True)
    assert sorted(i for grp in groups for i in grp) == list(range(6)) and len(words) == len(groups)


def test_fuzz_target_source_unchanged_by_name():
    src = open(Hh.__file__.replace("helpers.py", "native/fuzz_host.cpp")).read()
    assert "cw_collate_feed" in src and "cw_collate_get_token_groups" not in src
