"""The walk of align_long (generation.align_long, CrisperWhisperPipeline.align_long) over a scripted engine: which windows are
cut from the recording, what each is offered, where the cuts may fall, how seek and pos advance, the offsets on the timestamps,
the lockstep of several recordings, the trace and the refusals.  No GPU.

The scripted engine returns prescribed cuts and puts 0.06 s on every kept token (three 20 ms frames), so a window that keeps c
tokens ends its last word at 0.06 c s and the next window starts 3 c frames = 960 c samples later: with words of three tokens,
word m of the transcript comes out at (0.18 m, 0.18 (m + 1)) s wherever the cuts fall.  The recordings hold their own sample
index (recording B: plus 4 000 000; exact in float32), so a window tells the seek it was cut at."""
import math

import numpy as np
import pytest

from crisperwhisper_amd import collate, generation
from crisperwhisper_amd.pipeline import CrisperWhisperPipeline
from tests import helpers as Hh

SR = 16000
WIN = 30 * SR
B_OFF = 4_000_000


@pytest.fixture(scope="module")
def tiny():
    return Hh.tiny_setup()


class ScriptedEngine:
    """``script[rec]``: the cuts of recording ``rec``'s unforced windows, in order (a forced window takes all it is offered)."""

    def __init__(self, spec, script, max_batch=4):
        self.spec, self.max_batch = spec, max_batch
        self.script = {k: list(v) for k, v in script.items()}
        self.calls, self.clips = [], None

    def mel(self, clips):
        self.clips = [(int(c[0]) // B_OFF, int(c[0]) % B_OFF, len(c)) for c in clips]       # (recording, seek, samples)
        return None, np.array([(len(c) + 159) // 160 for c in clips], np.int32)

    def align_cut_tokens(self, num_frames, ids, n_init, cut_ok, force_all):
        assert len(ids) == len(self.clips) == len(cut_ok) == len(force_all) == len(num_frames)
        cuts, ts, lp = [], [], []
        for k, row in enumerate(ids):
            L = len(row) - n_init - 1
            assert len(cut_ok[k]) == L + 1 and row[-1] == self.spec.eos_token_id
            c = L if force_all[k] else self.script[self.clips[k][0]].pop(0)
            assert force_all[k] or cut_ok[k][c], (self.clips[k], c, list(cut_ok[k]))
            cuts.append(c)
            ts.append(np.concatenate([np.zeros(n_init), 0.06 * (np.arange(c) + 1), [0.06 * max(c, 1)]]).astype(np.float32))
            lp.append((-0.25 * (np.arange(L + 1) + 1)).astype(np.float32))
        self.calls.append({"clips": list(self.clips), "rows": [np.asarray(r).copy() for r in ids], "n_init": n_init,
                           "masks": [np.asarray(m).copy() for m in cut_ok], "forced": [bool(f) for f in force_all],
                           "nf": np.asarray(num_frames).copy(), "cuts": list(cuts)})
        z = [np.zeros(len(r) - n_init, np.float32) for r in ids]
        return (np.asarray(cuts, np.int64), np.asarray([-1.5 * (c + 1) for c in cuts], np.float32), ts, lp, z,
                [np.zeros(len(r) - n_init, np.int64) for r in ids], z)


def _pipe(spec, v, eng):
    p = object.__new__(CrisperWhisperPipeline)
    p.bundle = type("B", (), {"spec": spec})()
    p.vocab = collate.Vocabulary.from_synthetic(v)
    p.tokenizer = p.vocab
    p.sampling_rate = SR
    p.engine = eng
    p.stats = {}
    return p


def _ids(text):
    return [ord(c) for c in text]


def _rec(seconds, rec=0):
    return (np.arange(int(seconds * SR), dtype=np.float64) + rec * B_OFF).astype(np.float32)


WORDS8 = " ab cd ef gh ij kl mn op"                        # 8 words of 3 tokens


def _expect_words(text, chunks):
    words = text.split()
    assert [c["text"] for c in chunks] == [" " + w for w in words]
    for m, c in enumerate(chunks):
        assert c["timestamp"] == (round(0.18 * m, 2), round(0.18 * (m + 1), 2)), (m, c)


def test_interior_cuts_across_four_windows(tiny):
    g, v, W, spec = tiny
    eng = ScriptedEngine(spec, {0: [6, 9, 3, 6]})
    p = _pipe(spec, v, eng)
    out = p.align_long(_rec(100), _ids(WORDS8), language="<|en|>", return_scores=True)
    assert out["text"] == WORDS8
    _expect_words(WORDS8, out["chunks"])
    seeks = [c["clips"][0][1] for c in eng.calls]
    assert seeks == [0, 5760, 14400, 17280]                            # 960 samples per kept token: whole 20 ms frames
    assert all(c["clips"][0][2] == WIN for c in eng.calls) and all(c["forced"] == [False] for c in eng.calls)
    init = [v.sot, v.lang_id("en"), v.transcribe]
    T = _ids(WORDS8)
    pos = 0
    for call, cut in zip(eng.calls, [6, 9, 3, 6]):
        assert call["n_init"] == 3 and call["rows"][0].tolist() == init + T[pos:] + [v.eos]
        assert call["masks"][0].tolist() == [(n % 3 == 0) for n in range(len(T) - pos + 1)]     # word starts, 0 and N
        pos += cut
    # scores: -0.25 (i + 1) for the i-th token a window is offered; the eos once, after the last token
    lps = np.concatenate([-0.25 * (np.arange(c) + 1) for c in (6, 9, 3, 6)] + [[-0.25 * 7]])
    assert out["logprob"] == pytest.approx(lps.sum()) and out["avg_logprob"] == pytest.approx(lps.sum() / 25)
    assert [c["logprob"] for c in out["chunks"][:2]] == pytest.approx([-1.5, -3.75])
    assert p.stats["align_long"] == [
        {"item": 0, "seek_s": s / SR, "offered": o, "cut": c, "cut_score": -1.5 * (c + 1), "forced": False}
        for s, o, c in zip(seeks, (24, 18, 9, 6), (6, 9, 3, 6))]


def test_empty_window_skips_thirty_seconds(tiny):
    g, v, W, spec = tiny
    eng = ScriptedEngine(spec, {0: [0, 3, 0, 21]})
    out = _pipe(spec, v, eng).align_long(_rec(200), _ids(WORDS8), language="<|en|>")
    assert [c["clips"][0][1] for c in eng.calls] == [0, WIN, WIN + 2880, 2 * WIN + 2880]
    assert [c["text"] for c in out["chunks"]] == [" " + w for w in WORDS8.split()]
    assert out["chunks"][0]["timestamp"] == (30.0, 30.18)
    assert out["chunks"][1]["timestamp"] == (round(60.18, 2), round(60.36, 2))
    assert all(set(c) == {"text", "timestamp"} for c in out["chunks"])


def test_forced_last_window_takes_everything(tiny):
    g, v, W, spec = tiny
    eng = ScriptedEngine(spec, {0: [3, 0]})
    p = _pipe(spec, v, eng)
    out = p.align_long(_rec(40), _ids(WORDS8), language="<|en|>")
    assert [(c["clips"][0][1], c["forced"][0], c["cuts"][0]) for c in eng.calls] == [(0, False, 3), (2880, False, 0),
                                                                                    (WIN + 2880, True, 21)]
    assert eng.calls[2]["clips"][0][2] == 40 * SR - WIN - 2880          # the last window is what is left of the recording
    assert eng.calls[2]["nf"].tolist() == [(40 * SR - WIN - 2880 + 159) // 160]
    assert len(out["chunks"]) == 8 and out["chunks"][1]["timestamp"][0] == round((WIN + 2880) / SR, 2)
    assert [t["forced"] for t in p.stats["align_long"]] == [False, False, True]


def test_max_window_tokens_makes_several_passes_over_the_last_window(tiny):
    g, v, W, spec = tiny
    eng = ScriptedEngine(spec, {0: []})
    p = _pipe(spec, v, eng)
    out = p.align_long(_rec(10), _ids(WORDS8), language="<|en|>", max_window_tokens=16)
    # 16 is no word boundary: 15 tokens (five words), then the other nine; seek stays on the forced window
    assert [(c["clips"][0][1], len(c["rows"][0]) - 4, c["forced"][0]) for c in eng.calls] == [(0, 15, True), (0, 9, True)]
    assert [c["text"] for c in out["chunks"]] == [" " + w for w in WORDS8.split()]
    assert len(p.stats["align_long"]) <= 24 + math.ceil(10 / 30) + 1


def test_offer_is_rounded_down_to_a_word_start(tiny):
    g, v, W, spec = tiny
    text = " a bcdef gh i"                                             # word starts at 0, 2, 8, 11; N = 13
    eng = ScriptedEngine(spec, {0: [2, 6, 3, 2]})
    p = _pipe(spec, v, eng)
    out = p.align_long(_rec(100), _ids(text), language="<|en|>", max_window_tokens=7)
    # pos 0: 7 -> 2 (the next start, 8, is too far); pos 2: up to 9 -> 8; pos 8: up to 15 -> N = 13; pos 11: the last two
    assert [len(c["rows"][0]) - 4 for c in eng.calls] == [2, 6, 5, 2]
    assert eng.calls[0]["masks"][0].tolist() == [True, False, True]
    assert eng.calls[1]["masks"][0].tolist() == [True] + [False] * 5 + [True]
    assert eng.calls[2]["masks"][0].tolist() == [True, False, False, True, False, True]
    assert [c["text"] for c in out["chunks"]] == [" a", " bcdef", " gh", " i"]


def test_two_recordings_in_lockstep(tiny):
    g, v, W, spec = tiny
    short, long_ = " ab cd", WORDS8
    script = {0: [9, 15], 1: []}
    eng = ScriptedEngine(spec, script)
    p = _pipe(spec, v, eng)
    out = p.align_long([_rec(70, 0), _rec(12, 1)], [_ids(long_), _ids(short)], language="<|en|>", return_scores=True)
    assert [[c[0] for c in call["clips"]] for call in eng.calls] == [[0, 1], [0]]       # the short one finishes first
    assert eng.calls[0]["forced"] == [False, True] and eng.calls[0]["nf"].tolist() == [3000, 1200]
    alone0 = _pipe(spec, v, ScriptedEngine(spec, script)).align_long(_rec(70, 0), _ids(long_), language="<|en|>", return_scores=True)
    alone1 = _pipe(spec, v, ScriptedEngine(spec, script)).align_long(_rec(12, 1), _ids(short), language="<|en|>", return_scores=True)
    assert out == [alone0, alone1]
    assert [t["item"] for t in p.stats["align_long"]] == [0, 1, 0]
    # more recordings than decoder rows: successive groups
    eng2 = ScriptedEngine(spec, {0: [], 1: []}, max_batch=1)
    p2 = _pipe(spec, v, eng2)
    two = p2.align_long([_rec(5, 0), _rec(6, 1)], [_ids(short), _ids(short)], language="<|en|>")
    assert [[c[0] for c in call["clips"]] for call in eng2.calls] == [[0], [1]] and two[0] == two[1]
    assert [t["item"] for t in p2.stats["align_long"]] == [0, 1]


def test_empty_transcript_does_not_touch_the_engine(tiny):
    g, v, W, spec = tiny

    class Untouchable:
        spec_ = spec
        max_batch = 2

        def __getattr__(self, name):
            if name == "spec":
                return self.spec_
            raise AssertionError("the engine was touched: " + name)
    out = _pipe(spec, v, Untouchable()).align_long(_rec(50), [], language="<|en|>", return_scores=True)
    assert out["text"] == "" and out["chunks"] == []


def test_refusals(tiny):
    g, v, W, spec = tiny
    eng = ScriptedEngine(spec, {0: []})
    p = _pipe(spec, v, eng)
    x = _rec(40)
    with pytest.raises(ValueError, match="above the 2"):                # a word longer than the cap
        p.align_long(x, _ids(" ab cd"), language="<|en|>", max_window_tokens=2)
    with pytest.raises(ValueError, match="timestamp token"):
        p.align_long(x, [32, 97, v.timestamp_begin + 5], language="<|en|>")
    with pytest.raises(ValueError, match="special"):
        p.align_long(x, [32, v.eos], language="<|en|>")
    with pytest.raises(ValueError, match="2 transcripts"):
        p.align_long([x, x], [[32, 97]], language="<|en|>")
    with pytest.raises(ValueError, match="max_window_tokens"):
        p.align_long(x, [32, 97], language="<|en|>", max_window_tokens=0)
    with pytest.raises(ValueError, match="max_window_tokens"):
        p.align_long(x, [32, 97], language="<|en|>", max_window_tokens=g.max_target_positions)
    with pytest.raises(ValueError, match="token ids"):
        p.align_long(x, "hello", language="<|en|>")
    with pytest.raises(ValueError, match="rows"):
        generation.align_long(eng, [x] * 5, [[32, 97]] * 5, None, language="<|en|>")
    assert eng.calls == []


def test_walk_ends_within_tokens_plus_windows_rounds(tiny):
    """The slowest walk: every unforced window keeps nothing or a single one-token word."""
    g, v, W, spec = tiny
    text = " " + " ".join("abcdefgh")                                   # 8 words of 2 tokens -> N = 16
    n_tok = len(_ids(text))
    cuts = [0, 2, 0, 2, 2, 0, 0]
    eng = ScriptedEngine(spec, {0: cuts})
    p = _pipe(spec, v, eng)
    out = p.align_long(_rec(125), _ids(text), language="<|en|>")
    rounds = len(p.stats["align_long"])
    assert rounds <= n_tok + math.ceil(125 / 30) + 1
    assert sum(t["cut"] for t in p.stats["align_long"]) == n_tok and p.stats["align_long"][-1]["forced"]
    assert "".join(c["text"] for c in out["chunks"]) == text
