"""Host logic of forced alignment (generation.align, CrisperWhisperPipeline.align): transcript checks, init tokens, the rows
handed to the engine and the refusals that come before any device work.  No GPU: a stand-in engine records the call."""
import numpy as np
import pytest

from crisperwhisper_amd import collate, generation, synthetic as syn
from crisperwhisper_amd.pipeline import CrisperWhisperPipeline
from tests import helpers as Hh


@pytest.fixture(scope="module")
def tiny():
    return Hh.tiny_setup()


class FakeEngine:
    def __init__(self, spec, max_batch=4):
        self.spec, self.max_batch, self.calls = spec, max_batch, []

    def align_tokens(self, num_frames, ids, n_init):
        self.calls.append(([np.asarray(r).copy() for r in ids], n_init, np.asarray(num_frames).copy()))
        return [np.arange(len(r), dtype=np.float32) * 0.02 for r in ids]


def _pipe(spec, v, tokenizer=None):
    p = object.__new__(CrisperWhisperPipeline)
    p.bundle = type("B", (), {"spec": spec})()
    p.vocab = collate.Vocabulary.from_synthetic(v)
    p.tokenizer = tokenizer if tokenizer is not None else p.vocab
    p.sampling_rate = 16000
    p.engine = None
    return p


def test_generation_align_rows_and_slices(tiny):
    g, v, W, spec = tiny
    eng = FakeEngine(spec)
    out = generation.align(eng, 2, [3000, 1200], [[5, 6, 7], np.array([8])], language="<|en|>", task="transcribe")
    rows, n_init, nf = eng.calls[0]
    init = [v.sot, v.lang_id("en"), v.transcribe]
    assert n_init == 3 and nf.tolist() == [3000, 1200]
    assert rows[0].tolist() == init + [5, 6, 7, v.eos] and rows[1].tolist() == init + [8, v.eos]
    assert [s.tolist() for s in out["sequences"]] == [[5, 6, 7], [8]]
    assert np.allclose(out["token_timestamps"][0], [0.06, 0.08, 0.10]) and np.allclose(out["token_timestamps"][1], [0.06])


def test_transcript_id_checks(tiny):
    g, v, W, spec = tiny
    ok = generation.check_transcript_ids(spec, [1, 2, v.timestamp_begin + 3])     # timestamp tokens are kept
    assert ok.dtype == np.int64 and ok.tolist() == [1, 2, v.timestamp_begin + 3]
    for bad, word in [([v.eos], "special"), ([v.sot], "special"), ([v.notimestamps], "special"), ([g.vocab], "vocabulary"),
                      ([-1], "vocabulary"), ([[1, 2]], "1-D"), ([1.5], "integer")]:
        with pytest.raises(ValueError, match=word):
            generation.check_transcript_ids(spec, bad)
    with pytest.raises(TypeError):
        generation.check_transcript_ids(spec, "text")


def test_generation_align_refusals(tiny):
    g, v, W, spec = tiny
    eng = FakeEngine(spec, max_batch=2)
    with pytest.raises(ValueError, match="max_target_positions"):
        generation.align(eng, 1, [3000], [[5] * (g.max_target_positions - 3)], language="<|en|>")
    with pytest.raises(ValueError, match="rows"):
        generation.align(eng, 3, [3000] * 3, [[5]] * 3, language="<|en|>")
    with pytest.raises(ValueError, match="transcripts"):
        generation.align(eng, 2, [3000] * 2, [[5]], language="<|en|>")
    assert eng.calls == []


def test_pipeline_align_refusals_before_device_work(tiny):
    g, v, W, spec = tiny
    p = _pipe(spec, v)
    x = np.zeros(16000, np.float32)
    with pytest.raises(ValueError, match="token ids"):                   # str with the native Vocabulary
        p.align(x, "hello world", language="<|en|>")
    with pytest.raises(ValueError, match="prompt_ids"):
        p.align(x, [5], language="<|en|>", prompt_ids=[1, 2])
    with pytest.raises(ValueError, match="prompt_ids"):
        p.align(x, [5], generate_kwargs={"language": "<|en|>", "prompt_ids": [1, 2]})
    with pytest.raises(ValueError, match="2 transcripts"):
        p.align([x, x], [[5]], language="<|en|>")
    with pytest.raises(ValueError, match="special"):
        p.align(x, [5, v.eos], language="<|en|>")
    with pytest.raises(ValueError, match="vocabulary"):
        p.align(x, [g.vocab + 1], language="<|en|>")
    with pytest.raises(ValueError, match="30 s"):
        p.align(np.zeros(480001, np.float32), [5], language="<|en|>")
    with pytest.raises(ValueError, match="30 s"):
        p.align({"array": np.zeros(480001, np.float32), "sampling_rate": 16000}, [5], language="<|en|>")
    with pytest.raises(TypeError):
        p.align(x, [5], bogus=1)


def test_pipeline_align_encodes_str_with_a_tokenizer(tiny):
    g, v, W, spec = tiny

    class Tok:
        def __init__(self):
            self.seen = []

        def encode(self, text, add_special_tokens=True):
            self.seen.append((text, add_special_tokens))
            return [7, 8, 9]
    tok = Tok()
    p = _pipe(spec, v, tokenizer=tok)
    assert p._transcript_ids("Dr. Nguyen").tolist() == [7, 8, 9]
    assert tok.seen == [("Dr. Nguyen", False)]


def test_align_output_schema_through_adjust_pauses(tiny):
    """CrisperWhisperPipeline.align over a stand-in engine: one dict per input with __call__'s word schema, words collated from the
    transcript's ids and the engine's timestamps (init tokens and eos dropped); adjust_pauses_for_hf_pipeline_output takes it."""
    import crisperwhisper_amd as cw
    g, v, W, spec = tiny

    class StandIn(FakeEngine):
        def mel(self, clips):
            return None, np.array([(len(c) + 159) // 160 for c in clips], np.int32)

        def adjust_pauses(self, start, end, thr):
            return start, end
    eng = StandIn(spec, max_batch=2)
    p = _pipe(spec, v)
    p.engine = eng
    ids = [[32, 97, 98, 32, 99], [32, 100]]                            # " ab c", " d"
    out = p.align([np.zeros(16000, np.float32), np.zeros(8000, np.float32), np.zeros(4000, np.float32)],
                  ids + [[32, 101, 102]], language="<|en|>")
    assert [len(c[0]) for c in eng.calls] == [2, 1]                    # batches of the engine's rows
    assert eng.calls[0][2].tolist() == [100, 50]
    assert [o["text"] for o in out] == [" ab c", " d", " ef"]
    assert [w["text"] for w in out[0]["chunks"]] == [" ab", " c"]
    # the stand-in puts 0.02 s per position; the transcript's tokens are positions 3 .. 7 of init + text + eos
    want = collate.decode_asr(p.vocab, [{"tokens": np.array(ids[0]), "token_timestamps": np.arange(3, 8, dtype=np.float32) * 0.02}])
    assert (out[0]["text"], out[0]["chunks"]) == want
    one = p.align(np.zeros(16000, np.float32), ids[0], language="<|en|>")
    assert isinstance(one, dict) and set(one) == {"text", "chunks"}
    res = cw.adjust_pauses_for_hf_pipeline_output(one, engine=eng)
    assert res is one and all(set(c) == {"text", "timestamp"} for c in one["chunks"])
