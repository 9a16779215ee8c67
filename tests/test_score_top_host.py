"""Host plumbing of top_logprobs on the teacher-forced side (generation.score / align / align_long, CrisperWhisperPipeline.score /
align / align_long, Engine._with_score_top) over stand-in engines: output shapes, "rank", the kept prefix of align_long's windows,
top_logprobs=0 / None giving today's results exactly, refusals before the engine or the audio is touched, and the switch being
cleared when the call raises.  No GPU."""
import ctypes

import numpy as np
import pytest

from crisperwhisper_amd import _native, collate, generation
from crisperwhisper_amd.engine import Engine
from crisperwhisper_amd.pipeline import CrisperWhisperPipeline, token_alternatives
from tests import helpers as Hh

SR = 16000


@pytest.fixture(scope="module")
def tiny():
    return Hh.tiny_setup()


def _alts(rows, n_init, k):
    """Alternatives that tell their row and place: position j of a row lists ids (target + 1, target, target + 2, ...) -- the
    target at rank 1 -- except position 0, which lists ids from 200 on (the target is not among them), and the last k - 2 ranks
    of position 1, which are empty (-1 / NaN)."""
    ai, al = [], []
    for r in rows:
        tg = np.asarray(r[n_init:], np.int64)
        a = np.stack([np.concatenate([[t + 1, t], t + 2 + np.arange(k - 2)])[:k] if k > 1 else np.asarray([t + 1]) for t in tg])
        l = np.stack([-(np.arange(k) + 1) / 4.0 - j for j in range(len(tg))]).astype(np.float32)
        a[0] = 200 + np.arange(k)
        if len(tg) > 1 and k > 2:
            a[1, 2:] = -1
            l[1, 2:] = np.nan
        ai.append(a)
        al.append(l)
    return ai, al


class FakeEngine:
    """Scores like tests/test_score_host.py's stand-in; the log-probability of a target at rank 1 is that rank's."""

    def __init__(self, spec, max_batch=4, cuts=None):
        self.spec, self.max_batch, self.calls, self.mels, self.cuts = spec, max_batch, [], [], list(cuts or [])

    def mel(self, clips):
        self.mels.append([len(c) for c in clips])
        return None, np.asarray([min(3000, len(c) // 160) for c in clips])

    def _scores(self, rows, n_init, top):
        lp = [(-(np.arange(len(r) - n_init) + 1) / 8.0 - np.asarray(r[n_init:]) / 1024.0).astype(np.float32) for r in rows]
        out = (lp, [np.asarray(r[n_init:], np.int64) for r in rows], [a / 2 for a in lp])
        return out + (tuple(_alts(rows, n_init, top)) if top else ())

    def score_tokens(self, rows, n_init, rows_per_item=1, top_logprobs=0):
        self.calls.append(("score", len(rows), rows_per_item, top_logprobs))
        return self._scores(rows, n_init, top_logprobs)

    def align_score_tokens(self, num_frames, ids, n_init, top_logprobs=0):
        self.calls.append(("align_score", len(ids), 1, top_logprobs))
        return ([np.arange(len(r), dtype=np.float32) * 0.02 for r in ids],) + self._scores(ids, n_init, top_logprobs)

    def align_tokens(self, num_frames, ids, n_init):
        self.calls.append(("align", len(ids), 1, 0))
        return [np.arange(len(r), dtype=np.float32) * 0.02 for r in ids]

    def align_cut_tokens(self, num_frames, ids, n_init, cut_ok, force_all, top_logprobs=0):
        self.calls.append(("align_cut", len(ids), 1, top_logprobs))
        cuts = [len(r) - n_init - 1 if f else self.cuts.pop(0) for r, f in zip(ids, force_all)]
        ts = [np.concatenate([np.zeros(n_init), 0.06 * (np.arange(c) + 1), [0.06 * max(c, 1)]]).astype(np.float32) for c in cuts]
        lp, ti, tl, *alts = self._scores(ids, n_init, top_logprobs)
        return (np.asarray(cuts, np.int64), np.zeros(len(ids), np.float32), ts, lp, [np.zeros_like(a) for a in lp], ti, tl) + tuple(alts)


def _pipe(spec, v, eng):
    p = object.__new__(CrisperWhisperPipeline)
    p.bundle = type("B", (), {"spec": spec})()
    p.vocab = collate.Vocabulary.from_synthetic(v)
    p.tokenizer = p.vocab
    p.sampling_rate = SR
    p.engine = eng
    p.engines = [eng]
    p.stats = {}
    return p


KW = dict(language="<|en|>", task="transcribe")
TEXT = [ord(c) for c in " ab cd"]


def test_exported_symbols_and_prototypes():
    lib = _native.load()
    for name, n_args in (("cw_set_score_top_logprobs", 2), ("cw_get_score_top_logprobs", 5), ("cw_test_score_head_top", 16),
                         ("cw_test_score_head_stop_top", 19), ("cw_test_score_rows_top", 15), ("cw_time_score_head_top", 6)):
        assert name in _native.exported_symbols()
        assert len(getattr(lib, name).argtypes) == n_args and getattr(lib, name).restype is ctypes.c_int32
    assert len(lib.cw_score_tokens.argtypes) == 10 and len(lib.cw_align_score_tokens.argtypes) == 11      # signatures kept
    assert len(lib.cw_align_cut_tokens.argtypes) == 16 and len(lib.cw_time_score_head.argtypes) == 5
    header = open(Hh.ROOT + "/include/crisperwhisper.h").read()
    for name in ("cw_set_score_top_logprobs", "cw_get_score_top_logprobs", "cw_test_score_head_top", "cw_test_score_head_stop_top",
                 "cw_test_score_rows_top", "cw_time_score_head_top"):
        assert name + "(" in header


def test_generation_score_carries_the_alternatives(tiny):
    g, v, W, spec = tiny
    eng = FakeEngine(spec)
    plain = generation.score(eng, 1, [[[5, 6, 7], [8]]], **KW)
    none = generation.score(eng, 1, [[[5, 6, 7], [8]]], top_logprobs=None, **KW)
    zero = generation.score(eng, 1, [[[5, 6, 7], [8]]], top_logprobs=0, **KW)
    assert [c[3] for c in eng.calls] == [0, 0, 0]
    for a, b in ((plain, none), (plain, zero)):
        assert [sorted(o) for o in a[0]] == [sorted(o) for o in b[0]] == [["ids", "token_logprobs", "top_ids", "top_logprobs"]] * 2
        assert all(np.array_equal(x[key], y[key]) for x, y in zip(a[0], b[0]) for key in x)
    out = generation.score(eng, 1, [[[5, 6, 7], [8]]], top_logprobs=3, **KW)
    assert eng.calls[-1] == ("score", 2, 2, 3)
    for o, p_ in zip(out[0], plain[0]):
        assert all(np.array_equal(o[key], p_[key]) for key in p_)                   # "top_logprobs" keeps meaning the top-1 array
        n = len(o["ids"]) + 1
        assert o["alt_ids"].shape == (n, 3) and o["alt_logprobs"].shape == (n, 3)
        assert o["alt_ids"][1, 1] == (list(o["ids"]) + [v.eos])[1]
    for bad in (9, -1, 2.0, True, "3"):
        with pytest.raises(ValueError, match="top_logprobs"):
            generation.score(eng, 1, [[[5]]], top_logprobs=bad, **KW)


def test_generation_align_needs_return_scores(tiny):
    g, v, W, spec = tiny
    eng = FakeEngine(spec)
    with pytest.raises(ValueError, match="return_scores"):
        generation.align(eng, 1, [100], [[5, 6]], top_logprobs=2, **KW)
    with pytest.raises(ValueError, match="top_logprobs"):
        generation.align(eng, 1, [100], [[5, 6]], return_scores=True, top_logprobs=9, **KW)
    assert eng.calls == []
    out = generation.align(eng, 1, [100], [[5, 6]], return_scores=True, top_logprobs=2, **KW)
    assert eng.calls == [("align_score", 1, 1, 2)] and out["alt_ids"][0].shape == (3, 2) and out["alt_logprobs"][0].shape == (3, 2)
    plain = generation.align(eng, 1, [100], [[5, 6]], return_scores=True, **KW)
    assert sorted(plain) == ["sequences", "token_logprobs", "token_timestamps", "top_ids", "top_logprobs"]
    assert all(np.array_equal(out[key][0], plain[key][0]) for key in plain)


def test_pipeline_score_tokens_gain_alternatives_and_rank(tiny):
    g, v, W, spec = tiny
    eng = FakeEngine(spec)
    p = _pipe(spec, v, eng)
    x = np.zeros(SR, np.float32)
    plain = p.score(x, TEXT, **KW)
    assert p.score(x, TEXT, top_logprobs=0, **KW) == plain and p.score(x, TEXT, top_logprobs=None, **KW) == plain
    assert all(set(t) == {"id", "logprob", "top_id", "top_logprob"} for t in plain["tokens"])
    out = p.score(x, TEXT, top_logprobs=4, **KW)
    assert {key: out[key] for key in out if key != "tokens"} == {key: plain[key] for key in plain if key != "tokens"}
    toks = out["tokens"]
    assert [{key: t[key] for key in ("id", "logprob", "top_id", "top_logprob")} for t in toks] == plain["tokens"]
    assert toks[0]["rank"] is None and [e["id"] for e in toks[0]["top_logprobs"]] == [200, 201, 202, 203]
    assert len(toks[1]["top_logprobs"]) == 2 and toks[1]["rank"] == 1                    # the -1 entries are left out
    for j, t in enumerate(toks[2:], 2):
        assert t["rank"] == 1 and [e["id"] for e in t["top_logprobs"]] == [t["id"] + 1, t["id"], t["id"] + 2, t["id"] + 3]
        assert [e["logprob"] for e in t["top_logprobs"]] == [-0.25 - j, -0.5 - j, -0.75 - j, -1.0 - j]
        assert t["top_logprobs"][1]["text"] == chr(t["id"]) if t["id"] < 128 else True
    assert toks[-1]["id"] == v.eos and toks[-1]["top_logprobs"][1]["text"] == "<|endoftext|>"
    many = p.score([x, x], [[TEXT, TEXT[:3]], TEXT], top_logprobs=1, **KW)
    assert all(len(t["top_logprobs"]) == 1 and t["rank"] is None for t in many[0][1]["tokens"])


def test_token_alternatives():
    vocab = type("V", (), {"token_bytes": [b"a", b"b", b"c"], "specials": {}})()
    top, rank = token_alternatives(vocab, 1, np.asarray([2, 1, -1]), np.asarray([-0.5, -1.0, np.nan], np.float32))
    assert top == [{"id": 2, "text": "c", "logprob": -0.5}, {"id": 1, "text": "b", "logprob": -1.0}] and rank == 1
    assert token_alternatives(vocab, 0, np.asarray([-1, -1]), np.asarray([np.nan, np.nan], np.float32)) == ([], None)


def test_pipeline_align_chunks_gain_tokens(tiny):
    g, v, W, spec = tiny
    eng = FakeEngine(spec)
    p = _pipe(spec, v, eng)
    x = np.zeros(SR, np.float32)
    plain = p.align(x, TEXT, return_scores=True, **KW)
    assert p.align(x, TEXT, return_scores=True, top_logprobs=0, **KW) == plain
    out = p.align(x, TEXT, return_scores=True, top_logprobs=3, **KW)
    assert eng.calls[-1] == ("align_score", 1, 1, 3)
    assert [{key: c[key] for key in c if key != "tokens"} for c in out["chunks"]] == plain["chunks"]
    assert {key: out[key] for key in out if key != "chunks"} == {key: plain[key] for key in plain if key != "chunks"}
    assert [[t["id"] for t in c["tokens"]] for c in out["chunks"]] == [TEXT[:3], TEXT[3:]]       # the collator's own groups
    sc = p.score(x, TEXT, top_logprobs=3, **KW)
    flat = [t for c in out["chunks"] for t in c["tokens"]]
    for t, s in zip(flat, sc["tokens"]):
        assert set(t) == {"id", "text", "logprob", "top_logprobs", "rank"}
        assert (t["id"], t["logprob"], t["top_logprobs"], t["rank"]) == (s["id"], s["logprob"], s["top_logprobs"], s["rank"])
    assert flat[0]["text"] == " " and flat[1]["text"] == "a"
    assert [c["logprob"] for c in out["chunks"]] == pytest.approx([sum(t["logprob"] for t in c["tokens"]) for c in out["chunks"]])


def test_refusals_come_before_the_engine_and_the_audio(tiny):
    g, v, W, spec = tiny
    eng = FakeEngine(spec)
    p = _pipe(spec, v, eng)

    class NoAudio:                                               # an input that must not be loaded
        def __array__(self, *a, **k):
            raise AssertionError("the audio was touched")
    x = NoAudio()
    for bad in (9, -1, 1.5, True, "2"):
        for fn, kw in ((p.score, {}), (p.align, {"return_scores": True}), (p.align_long, {"return_scores": True})):
            with pytest.raises(ValueError, match="top_logprobs"):
                fn(x, TEXT, top_logprobs=bad, **kw, **KW)
    for fn in (p.align, p.align_long):
        with pytest.raises(ValueError, match="return_scores=True"):
            fn(x, TEXT, top_logprobs=2, **KW)
    assert eng.calls == [] and eng.mels == []


def test_align_long_keeps_the_kept_prefix_rows(tiny):
    g, v, W, spec = tiny
    text = " ab cd ef gh"                                        # 4 words of 3 tokens
    T = [ord(c) for c in text]
    # 0.06 s per kept token: the windows start at 0, 5760 and 8640 samples, and only the third reaches the end of 30.4 s
    rec = np.zeros(486400, np.float32)
    plain_eng = FakeEngine(spec, cuts=[6, 3])
    plain = _pipe(spec, v, plain_eng).align_long(rec, T, return_scores=True, **KW)
    eng = FakeEngine(spec, cuts=[6, 3])
    p = _pipe(spec, v, eng)
    out = p.align_long(rec, T, return_scores=True, top_logprobs=3, **KW)
    assert [c[3] for c in eng.calls] == [3, 3, 3] and [c[3] for c in plain_eng.calls] == [0, 0, 0]
    assert [{key: c[key] for key in c if key != "tokens"} for c in out["chunks"]] == plain["chunks"]
    assert {key: out[key] for key in out if key != "chunks"} == {key: plain[key] for key in plain if key != "chunks"}
    assert all("tokens" not in c for c in plain["chunks"])
    assert [[t["id"] for t in c["tokens"]] for c in out["chunks"]] == [T[0:3], T[3:6], T[6:9], T[9:12]]
    # window 1 is offered 12 tokens and keeps 6 (its rows 0 .. 5), window 2 is offered 6 and keeps 3, the last takes 3: a token's
    # alternatives are those of its place in its own window -- place 0 lists 200 .., place 1 two entries, the others rank 1
    place = [0, 1, 2, 3, 4, 5, 0, 1, 2, 0, 1, 2]
    flat = [t for c in out["chunks"] for t in c["tokens"]]
    for t, j in zip(flat, place):
        assert set(t) == {"id", "text", "logprob", "top_logprobs", "rank"}
        assert t["logprob"] == float(np.float32(-(j + 1) / 8.0 - t["id"] / 1024.0))
        if j == 0:
            assert t["rank"] is None and [e["id"] for e in t["top_logprobs"]] == [200, 201, 202]
        elif j == 1:
            assert t["rank"] == 1 and [e["id"] for e in t["top_logprobs"]] == [t["id"] + 1, t["id"]]
        else:
            assert t["rank"] == 1 and [e["logprob"] for e in t["top_logprobs"]] == [-0.25 - j, -0.5 - j, -0.75 - j]


def test_engine_switch_is_cleared_when_the_call_raises():
    class Lib:
        def __init__(self):
            self.set, self.fail_get = [], False

        def cw_set_score_top_logprobs(self, ctx, k):
            self.set.append(k)
            return 0

        def cw_get_score_top_logprobs(self, ctx, ids, lp, rows, stride):
            return 1 if self.fail_get else 0
    eng = object.__new__(Engine)
    eng.lib, eng.ctx = Lib(), None

    def chk(code):
        if code:
            raise RuntimeError("engine error")
    eng._chk = chk
    n = np.asarray([5, 4], np.int32)

    def boom():
        raise RuntimeError("the call failed")
    with pytest.raises(RuntimeError, match="the call failed"):
        eng._with_score_top(3, boom, 2, 6, n, 3)
    assert eng.lib.set == [3, 0]
    eng.lib.fail_get = True
    with pytest.raises(RuntimeError, match="engine error"):
        eng._with_score_top(2, lambda: None, 2, 6, n, 3)
    assert eng.lib.set == [3, 0, 2, 0]
    eng.lib.fail_get = False
    ai, al = eng._with_score_top(8, lambda: None, 2, 6, n, 3)
    assert eng.lib.set[-2:] == [8, 0] and [a.shape for a in ai] == [(2, 8), (1, 8)] and al[0].dtype == np.float32
    for bad in (0, 9):
        with pytest.raises(ValueError):
            eng._with_score_top(bad, boom, 2, 6, n, 3)
    assert eng.lib.set[-2:] == [8, 0]
