"""Host side of the alignment scores: the exported symbols and prototypes, the pipeline's refusals, and the way the per-token
arrays reach the words -- through segment slicing, long-form seam merging and the sharded gather -- over a scripted engine.
Host-only: no GPU."""
import ctypes
import math

import numpy as np
import pytest

from crisperwhisper_amd import _native, collate, dist, generation, synthetic as syn
from crisperwhisper_amd.pipeline import CrisperWhisperPipeline, add_alignment_scores
from tests import alignment_score_refs as R
from tests import helpers as Hh

NEW = ("cw_set_alignment_scores", "cw_get_alignment_scores", "cw_get_transcribe_alignment_scores", "cw_test_align_path_scores")


def test_exported_symbols_and_prototypes():
    lib = _native.load()
    header = open(Hh.ROOT + "/include/crisperwhisper.h").read()
    for name in NEW:
        assert name in _native.exported_symbols()
        assert getattr(lib, name).restype is ctypes.c_int32
        assert name + "(" in header
    assert len(lib.cw_set_alignment_scores.argtypes) == 3
    assert len(lib.cw_get_alignment_scores.argtypes) == 5
    assert len(lib.cw_get_transcribe_alignment_scores.argtypes) == 5
    assert len(lib.cw_test_align_path_scores.argtypes) == 11
    assert lib.cw_abi_version() == 1
    assert len(lib.cw_token_timestamps.argtypes) == 6 and len(lib.cw_align_tokens.argtypes) == 8      # signatures kept


def _window(v, words, t0, t1):
    """One window's tokens <|t0|> words... <|t1|> over the byte vocabulary, timestamps spread over (t0, t1)."""
    tb = v.timestamp_begin
    toks = [tb + int(round(t0 / 0.02))] + [b for w in words for b in (" " + w).encode()] + [tb + int(round(t1 / 0.02))]
    return np.asarray(toks, np.int64), np.linspace(t0, t1, len(toks)).astype(np.float32)


# ---- a scripted engine: window k of the recording decodes to SCRIPT[k] ---------------------------------------------------
def _script(v):
    """Three 30 s windows of one recording whose texts overlap at the seams, with per-token values that name the token:
    mass = 1 / (2 + global index), spread = 0.001 * (1 + global index)."""
    spans = [(["ab", "cd", "ef", "gh"], 0.0, 29.0), (["ef", "gh", "ij", "kl"], 1.0, 20.0), (["ij", "kl", "mn", "op"], 1.0, 14.0)]
    out, n0 = [], 0
    for words, t0, t1 in spans:
        tok, ts = _window(v, words, t0, t1)
        idx = n0 + np.arange(len(tok))
        out.append((tok, ts, (1.0 / (2 + idx)).astype(np.float32), (0.001 * (1 + idx)).astype(np.float32)))
        n0 += len(tok)
    return out


class ScriptedEngine:
    """``mel`` is handed the clips of one batch; the windows they are come from ``order`` (the windows this rank runs, in
    order).  The native seek loop (``transcribe``) returns the scripted tokens."""

    def __init__(self, spec, script, order, with_scores=True, on=False, beam_open=False):
        self.spec, self.script, self.order, self.max_batch = spec, script, list(order), 8
        self.calls, self.batch, self.on = [], [], on
        self.alignment_scores_on, self.beam_open = on, beam_open          # as Engine tracks it / as cw_beam_begin leaves it
        if with_scores:
            self.set_alignment_scores = self._set
            self.transcribe_alignment_scores = self._get

    def mel(self, clips):
        self.batch = [self.order.pop(0) for _ in clips]
        return None, np.asarray([min(3000, len(c) // 160) for c in clips])

    def _set(self, on, collar_frames=0):
        self.calls.append(("set_alignment_scores", bool(on), collar_frames))
        if on and self.beam_open:                            # cw_set_alignment_scores: switching on is refused, off never
            raise RuntimeError("set_alignment_scores: a beam search is open")
        self.on = self.alignment_scores_on = bool(on)

    def transcribe(self, nb, num_frames, **kw):
        assert nb == len(self.batch)
        self.beam_open = False                               # a decode closes a search that was left open
        return [self.script[k][0] for k in self.batch], [self.script[k][1] for k in self.batch], 1

    def _get(self, lens):
        assert self.on, "fetched while the switch is off"
        assert list(lens) == [len(self.script[k][0]) for k in self.batch]
        return [self.script[k][2] for k in self.batch], [self.script[k][3] for k in self.batch]


def _pipe(spec, v, eng, shard=None, batch_size=1, **attrs):
    p = object.__new__(CrisperWhisperPipeline)
    p.bundle = type("B", (), {"spec": spec})()
    p.vocab = collate.Vocabulary.from_synthetic(v)
    p.tokenizer = p.vocab
    p.sampling_rate = 16000
    p.engine, p.engines = eng, [eng]
    p.shard = shard or dist.Shard()
    p.batch_size, p.max_rows = batch_size, 8
    p.chunk_length_s, p.stride_length_s = 30, 5
    p.return_timestamps, p.return_scores, p.top_logprobs = "word", False, 0
    p.default_num_beams, p.sampling_seed, p.stats = 5, None, {}
    for a, x in attrs.items():
        setattr(p, a, x)
    return p


GK = {"num_beams": 1, "language": "<|en|>", "task": "transcribe"}
PCM = np.zeros(55 * 16000, np.float32)                       # windows at 0, 20 and 40 s


def _expected(v, script):
    vocab = collate.Vocabulary.from_synthetic(v)
    strides = [(30.0, 0.0, 5.0), (30.0, 5.0, 5.0), (15.0, 5.0, 0.0)]
    outputs = [{"tokens": s[0], "token_timestamps": s[1], "stride": st} for s, st in zip(script, strides)]
    text, words, groups = collate.decode_asr(vocab, outputs, time_precision=0.02, return_timestamps="word", return_token_groups=True)
    vals = R.word_scores(groups, np.concatenate([s[2] for s in script]), np.concatenate([s[3] for s in script]))
    return text, words, groups, vals


def test_long_form_seams_give_every_word_the_mean_of_its_own_tokens():
    g, v, W, spec = Hh.tiny_setup()
    script = _script(v)
    text, words, groups, vals = _expected(v, script)
    n_all = sum(len(s[0]) for s in script)
    flat = np.concatenate([s[0] for s in script])
    used = {int(i) for grp in groups for i in grp}
    dropped = {i for i in range(n_all) if flat[i] < v.eos} - used
    assert len(words) == 8 and dropped                        # the overlaps are decoded twice and kept once
    eng = ScriptedEngine(spec, script, [0, 1, 2])
    got = _pipe(spec, v, eng)(PCM, generate_kwargs=GK, return_alignment_scores=True)
    assert eng.calls and all(c == ("set_alignment_scores", True, spec.median_filter_width // 2) for c in eng.calls)
    assert got["text"] == text and len(got["chunks"]) == len(words)
    for c, w, grp, (m, s) in zip(got["chunks"], words, groups, vals):
        assert set(c) == {"text", "timestamp", "alignment_score", "alignment_spread"}
        assert c["text"] == w["text"] and c["timestamp"] == w["timestamp"]
        assert c["alignment_score"] == m and c["alignment_spread"] == s
        # the values name their tokens: a float64 mean over exactly this group, in which no dropped token takes part
        assert math.isclose(c["alignment_spread"], float(np.mean([np.float32(0.001 * (1 + i)) for i in grp], dtype=np.float64)),
                            rel_tol=1e-15)
        assert math.isclose(c["alignment_score"], float(np.mean([np.float32(1.0 / (2 + i)) for i in grp], dtype=np.float64)),
                            rel_tol=1e-15)
    # an explicit collar reaches the engine; the constructor's settings are the call's defaults
    eng = ScriptedEngine(spec, script, [0, 1, 2])
    again = _pipe(spec, v, eng, return_alignment_scores=True, alignment_collar_frames=7, batch_size=2)(PCM, generate_kwargs=GK)
    assert all(c == ("set_alignment_scores", True, 7) for c in eng.calls) and again == got
    # together with nothing else requested the other keys are as before; without the flag the chunks are the old ones
    eng = ScriptedEngine(spec, script, [0, 1, 2])
    plain = _pipe(spec, v, eng)(PCM, generate_kwargs=GK)
    assert eng.calls == []                                    # never on: a call without the flag does not touch the switch
    assert plain["text"] == text and all(set(c) == {"text", "timestamp"} for c in plain["chunks"])
    assert plain["chunks"] == [{"text": c["text"], "timestamp": c["timestamp"]} for c in got["chunks"]]
    # an engine without the switch still serves a call without the flag, and refuses one with it
    eng = ScriptedEngine(spec, script, [0, 1, 2], with_scores=False)
    assert _pipe(spec, v, eng)(PCM, generate_kwargs=GK) == plain
    with pytest.raises(ValueError, match="alignment scores"):
        _pipe(spec, v, ScriptedEngine(spec, script, [0, 1, 2], with_scores=False))(PCM, generate_kwargs=GK, return_alignment_scores=True)


def test_a_call_without_the_flag_is_served_whatever_state_the_engine_is_in():
    """An interrupted beam search leaves the engine with a search open, in which switching the scores on is refused.  A call
    without the flag never asks for that: on an engine that never had the switch on it does not touch it at all, and after a
    call with the flag it only switches it off, which is always accepted."""
    g, v, W, spec = Hh.tiny_setup()
    script = _script(v)
    want = _pipe(spec, v, ScriptedEngine(spec, script, [0, 1, 2]))(PCM, generate_kwargs=GK)
    eng = ScriptedEngine(spec, script, [0, 1, 2], beam_open=True)
    assert _pipe(spec, v, eng)(PCM, generate_kwargs=GK) == want and eng.calls == []
    eng = ScriptedEngine(spec, script, [0, 1, 2], on=True, beam_open=True)
    assert _pipe(spec, v, eng)(PCM, generate_kwargs=GK) == want
    assert eng.calls == [("set_alignment_scores", False, spec.median_filter_width // 2)] and eng.alignment_scores_on is False
    # generation.align likewise
    rec = _Recorder(spec)
    rec.align_tokens = lambda nf, ids, n_init: [np.zeros(len(r), np.float32) for r in ids]
    out = generation.align(rec, 1, [3000], [[5, 6]], language="<|en|>", task="transcribe")
    assert rec.calls == [] and "alignment_scores" not in out


class _Captured(Exception):
    pass


class _CaptureShard(dist.Shard):
    """Rank ``rank`` of ``world``: keeps what it would send and stops the call there."""

    def all_gather_records(self, recs, max_per_rank):
        self.sent, self.max_per_rank = recs, max_per_rank
        raise _Captured


class _ReplayShard(dist.Shard):
    """Rank 0 of ``world``: the gather returns what every rank sent, padded and ordered as the collective does."""

    def __init__(self, sent, world):
        super().__init__(0, world)
        self.all_sent = sent

    def all_gather_records(self, recs, max_per_rank):
        assert recs.tobytes() == self.all_sent[0].tobytes()
        width = recs.shape[1]
        bufs = []
        for s in self.all_sent:
            assert s.shape[1] == width                        # an empty shard sends the width the others send
            buf = np.full((max_per_rank, width), -1, np.int32)
            buf[:len(s)] = s
            bufs.append(buf)
        allr = np.concatenate(bufs)
        allr = allr[allr[:, 0] >= 0]
        return allr[np.argsort(allr[:, 0], kind="stable")]


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_gather_carries_the_arrays_to_the_same_words(world):
    g, v, W, spec = Hh.tiny_setup()
    script = _script(v)
    single = _pipe(spec, v, ScriptedEngine(spec, script, [0, 1, 2]))(PCM, generate_kwargs=GK, return_alignment_scores=True)
    bounds = dist.shard_bounds(3, world)
    sent = []
    for r, (lo, hi) in enumerate(bounds):                     # (world 4: the last rank has no window at all)
        sh = _CaptureShard(r, world)
        with pytest.raises(_Captured):
            _pipe(spec, v, ScriptedEngine(spec, script, range(lo, hi)), shard=sh)(PCM, generate_kwargs=GK, return_alignment_scores=True)
        assert sh.sent.shape == (hi - lo, dist.REC_WORDS + dist.REC_ALIGN_WORDS)
        sent.append(sh.sent)
    lo, hi = bounds[0]
    got = _pipe(spec, v, ScriptedEngine(spec, script, range(lo, hi)), shard=_ReplayShard(sent, world))(
        PCM, generate_kwargs=GK, return_alignment_scores=True)
    assert got == single


def test_the_tail_travels_behind_a_record_of_any_width():
    toks, ts, stride = np.array([1, 2, 300]), np.array([0.5, 1.25, 2.0], np.float32), (30.0, 5.0, 0.0)
    lp = np.array([-0.25, 0.0, -17.5], np.float32)
    mass, spread = np.array([1.0, 0.25, np.nan], np.float32), np.array([0.0, 0.5, np.nan], np.float32)
    top = (np.arange(6, dtype=np.int32).reshape(3, 2), -np.arange(6, dtype=np.float32).reshape(3, 2))
    for base in (dist.pack_record(7, toks, ts, stride), dist.pack_record(7, toks, ts, stride, lp),
                 dist.pack_record(7, toks, ts, stride, lp, top)):
        rec = dist.append_alignment(base, mass, spread)
        assert rec.dtype == np.int32 and rec.shape == (len(base) + dist.REC_ALIGN_WORDS,) and dist.REC_ALIGN_WORDS == 2 * dist.REC_TOKENS
        back, m2, s2 = dist.split_alignment(rec)
        assert back.tobytes() == base.tobytes() and m2.tobytes() == mass.tobytes() and s2.tobytes() == spread.tobytes()
        assert len(dist.unpack_record(back)) == len(dist.unpack_record(base))
    with pytest.raises(ValueError):
        dist.append_alignment(dist.pack_record(7, toks, ts, stride), mass[:2], spread[:2])
    with pytest.raises(ValueError):
        dist.split_alignment(dist.pack_record(7, toks, ts, stride))


def test_split_segments_cuts_the_scores_like_the_timestamps():
    tb = 1000
    seq = np.array([tb, 5, 6, tb + 10, tb + 10, 7, tb + 20, tb + 20, 8], np.int64)
    n_prompt = 3
    n = n_prompt + len(seq)
    ts, lp = np.arange(n, dtype=np.float32), -np.arange(n, dtype=np.float32)
    mass, spread = (np.arange(n) / 16).astype(np.float32), (np.arange(n) / 512).astype(np.float32)
    segs, adv = generation.split_segments(seq, ts, 0.0, tb, 3000, n_prompt, lp, None, (mass, spread))
    plain, adv2 = generation.split_segments(seq, ts, 0.0, tb, 3000, n_prompt, lp)
    assert adv == adv2 and len(segs) == len(plain) == 2
    for s, p in zip(segs, plain):
        a, b = s.idxs
        assert p.alignment_scores is None and p.alignment_spreads is None and s.idxs == p.idxs
        assert np.array_equal(s.token_logprobs, p.token_logprobs) and s.top_ids is None
        assert s.alignment_scores.dtype == np.float32 and np.array_equal(s.alignment_scores, mass[a:b])
        assert s.alignment_spreads.dtype == np.float32 and np.array_equal(s.alignment_spreads, spread[a:b])


def test_word_means_are_float64_and_nan_spreads():
    words = [{"text": " a"}, {"text": " b"}, {"text": " c"}]
    groups = [[0, 2], [3], []]
    add_alignment_scores(words, groups, [np.array([0.1, 9.0], np.float32), np.array([0.3, np.nan], np.float32)],
                         [np.array([0.5, 9.0], np.float32), np.array([0.25, 1.0], np.float32)])
    assert words[0]["alignment_score"] == (float(np.float32(0.1)) + float(np.float32(0.3))) / 2
    assert words[0]["alignment_spread"] == 0.375
    assert math.isnan(words[1]["alignment_score"]) and words[1]["alignment_spread"] == 1.0
    assert math.isnan(words[2]["alignment_score"]) and math.isnan(words[2]["alignment_spread"])


def test_pipeline_refusals_come_before_the_audio_is_loaded():
    """The input here is no audio at all: loading it raises TypeError."""
    g, v, W, spec = Hh.tiny_setup()
    p = _pipe(spec, v, None)
    with pytest.raises(ValueError, match="word"):
        p._run_one(12345, return_alignment_scores=True, return_timestamps=True, generate_kwargs=GK)      # segment mode
    p2 = _pipe(spec, v, None, return_alignment_scores=True)                                                # the constructor's value
    with pytest.raises(ValueError, match="word"):
        p2._run_one(12345, return_timestamps=True, generate_kwargs=GK)
    for bad in (-1, 2.5, "3", True):
        with pytest.raises(ValueError, match="alignment_collar_frames"):
            p._run_one(12345, return_alignment_scores=True, alignment_collar_frames=bad, generate_kwargs=GK)
        with pytest.raises(ValueError, match="alignment_collar_frames"):
            p.align(12345, [1, 2], return_alignment_scores=True, alignment_collar_frames=bad)
        with pytest.raises(ValueError, match="alignment_collar_frames"):
            generation.check_alignment_collar(spec, bad)
    assert generation.check_alignment_collar(spec, None) == spec.median_filter_width // 2
    assert generation.check_alignment_collar(spec, 0) == 0 and generation.check_alignment_collar(spec, np.int64(9)) == 9
    with pytest.raises(TypeError):
        p._run_one(12345, return_alignment_scores=True, alignment_collar_frames=4, generate_kwargs=GK)   # accepted: now it loads


class _Recorder:
    """An engine that records every call that would change its state."""

    def __init__(self, spec):
        self.spec, self.max_batch, self.calls = spec, 64, []

    def set_alignment_scores(self, on, collar_frames=0):
        self.calls.append(("set_alignment_scores", on, collar_frames))

    def __getattr__(self, name):
        raise AttributeError(f"engine.{name} reached by a call that must be refused")


def test_generate_and_align_refuse_a_bad_collar_before_the_engine_is_touched():
    g, v, W, spec = Hh.tiny_setup()
    eng = _Recorder(spec)
    with pytest.raises(ValueError, match="alignment_collar_frames"):
        generation.generate(eng, 1, [3000], language="<|en|>", task="transcribe", return_alignment_scores=True,
                            alignment_collar_frames=-2)
    with pytest.raises(ValueError, match="alignment_collar_frames"):
        generation.align(eng, 1, [3000], [[5, 6]], language="<|en|>", task="transcribe", return_alignment_scores=True,
                         alignment_collar_frames=1.5)
    assert eng.calls == []


class _AlignEngine:
    """``align_tokens`` with scripted timestamps; the scores of row b at position k are b + k / 64 and (b + k / 64) / 8."""

    def __init__(self, spec):
        self.spec, self.max_batch, self.calls = spec, 4, []

    def mel(self, clips):
        return None, np.asarray([min(3000, len(c) // 160) for c in clips])

    def set_alignment_scores(self, on, collar_frames=0):
        self.calls.append(("set", bool(on), collar_frames))
        self.alignment_scores_on = bool(on)

    def align_tokens(self, num_frames, ids, n_init):
        self.rows = [len(r) for r in ids]
        return [np.arange(len(r), dtype=np.float32) * 0.02 for r in ids]

    def alignment_scores(self, nb, L):
        assert nb == len(self.rows) and L == max(self.rows) - 1
        k = np.arange(L + 1)[None, :] / 64.0 + np.arange(nb)[:, None]
        return k.astype(np.float32), (k / 8).astype(np.float32)


def test_pipeline_align_adds_the_keys_over_its_own_groups():
    g, v, W, spec = Hh.tiny_setup()
    eng = _AlignEngine(spec)
    p = _pipe(spec, v, eng)
    texts = [list(b" ab cd"), list(b" efg")]
    clips = [np.zeros(16000, np.float32), np.zeros(32000, np.float32)]
    got = p.align(clips, texts, language="<|en|>", task="transcribe", return_alignment_scores=True)
    plain = p.align(clips, texts, language="<|en|>", task="transcribe")
    assert eng.calls == [("set", True, spec.median_filter_width // 2), ("set", False, spec.median_filter_width // 2)]
    assert p.align(clips, texts, language="<|en|>", task="transcribe") == plain and len(eng.calls) == 2      # off stays untouched
    n_init = 3
    for b, (r, q, t) in enumerate(zip(got, plain, texts)):
        assert r["text"] == q["text"]
        assert [{"text": c["text"], "timestamp": c["timestamp"]} for c in r["chunks"]] == q["chunks"]
        _, _, groups = collate.decode_asr(p.vocab, [{"tokens": np.asarray(t, np.int64), "token_timestamps": np.zeros(len(t), np.float32)}],
                                          time_precision=0.02, return_timestamps="word", return_token_groups=True)
        for c, grp in zip(r["chunks"], groups):
            want = float(np.mean([np.float32(b + (n_init + i) / 64.0) for i in grp], dtype=np.float64))
            assert set(c) == {"text", "timestamp", "alignment_score", "alignment_spread"}
            assert c["alignment_score"] == want and c["alignment_spread"] == want / 8
