"""Host side of word confidence: the beam host's per-token candidate log-probabilities (csrc/beamhost.cpp against the numpy
statement in generation.beam_search, on the candidate streams of tests/test_beam_host.py), word sums across a strided seam,
the gather record with and without scores, and the pipeline's argument check.  Host-only: no GPU."""
import numpy as np
import pytest

from crisperwhisper_amd import _native, collate, dist, generation, synthetic as syn
from crisperwhisper_amd.pipeline import CrisperWhisperPipeline, scored_words
from tests.test_beam_host import CASES, CandidateStream

U = 2.0 ** -24


def test_exported_symbols():
    for name in ("cw_set_token_logprobs", "cw_get_token_logprobs", "cw_get_transcribe_token_logprobs",
                 "cw_beam_host_token_logprobs", "cw_test_sample_logprobs"):
        assert name in _native.exported_symbols()
    lib = _native.load()
    assert lib.cw_abi_version() == 1
    assert lib.cw_beam_host_token_logprobs(None, None) != 0


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_beam_token_logprobs_follow_the_ancestry(case, seed):
    B, K, n_prompt, max_length, vocab, eos, pad, p_eos, lp, es = case
    eng = CandidateStream(100 * seed + B + K, B, K, vocab, eos, pad, p_eos, np.float32(0.25), max_length)
    prompt = np.random.default_rng(seed).integers(0, vocab, (B, n_prompt)).astype(np.int64)
    out = {}
    for native in (False, True):
        res = generation.beam_search(eng, prompt, max_length, 0, K, length_penalty=lp, early_stopping=es, native_host=native,
                                     return_token_logprobs=True)
        assert len(res) == 5
        plain = generation.beam_search(eng, prompt, max_length, 0, K, length_penalty=lp, early_stopping=es, native_host=native)
        assert len(plain) == 4 and np.array_equal(plain[0], res[0]) and np.array_equal(plain[1], res[1])
        out[native] = res
    seqs, bi, L, score, tl = out[True]
    tl0 = out[False][4]
    assert tl.dtype == np.float32 and tl0.dtype == np.float32 and tl.shape == bi.shape == tl0.shape
    assert np.array_equal(tl.view(np.uint32), tl0.view(np.uint32))               # native and numpy bookkeeping, bit for bit
    for b in range(B):
        n_gen = int((bi[b] != -1).sum())
        assert np.all(bi[b, :n_gen] != -1)
        assert np.all(np.isnan(tl[b, n_gen:])) and not np.any(np.isnan(tl[b, :n_gen]))      # NaN exactly behind the end
        for gpos in range(n_gen):                                                # the candidate value along the ancestry
            vals, toks = eng.steps[gpos]
            row = int(bi[b, gpos])
            j = np.nonzero(toks[row] == int(seqs[b, n_prompt + gpos]))[0]
            assert len(j) == 1
            assert tl[b, gpos].view(np.uint32) == vals[row, j[0]].view(np.uint32)
        if lp == 1.0 and score[b] > -1.0e8 and n_gen:
            # score = (f32 running sum of the candidate values) / f32(length): n_gen additions and one division, each one
            # rounding of a number no larger than sum |values|
            total = float(np.sum(tl[b, :n_gen].astype(np.float64)))
            mag = float(np.sum(np.abs(tl[b, :n_gen].astype(np.float64))))
            assert abs(total - float(score[b]) * n_gen) <= (n_gen + 2) * U * mag + 1e-30


def _window(v, words, t0, t1, first_id):
    """One window's tokens <|t0|> words... <|t1|> over the byte vocabulary, timestamps spread over (t0, t1), and per token the
    value -2^-(first_id + i): any subset of such values has a sum that names its members."""
    tb = v.timestamp_begin
    toks = [tb + int(round(t0 / 0.02))] + [b for w in words for b in (" " + w).encode()] + [tb + int(round(t1 / 0.02))]
    ts = np.linspace(t0, t1, len(toks)).astype(np.float32)
    lp = -(2.0 ** -(first_id + np.arange(len(toks)))).astype(np.float32)
    return np.asarray(toks, np.int64), ts, lp


def test_word_sums_across_a_strided_seam():
    g, v = syn.tiny_geometry()
    vocab = collate.Vocabulary.from_synthetic(v)
    a_tok, a_ts, a_lp = _window(v, ["ab", "cd", "ef", "gh"], 0.0, 29.0, 0)
    b_tok, b_ts, b_lp = _window(v, ["ef", "gh", "ij", "kl"], 1.0, 20.0, len(a_tok))
    outputs = [{"tokens": a_tok, "token_timestamps": a_ts, "stride": (30.0, 0.0, 5.0)},
               {"tokens": b_tok, "token_timestamps": b_ts, "stride": (30.0, 5.0, 0.0)}]
    n_all = len(a_tok) + len(b_tok)
    assert n_all < 50                                  # 2^-49 and its sums are exact in float64
    text, words = scored_words(vocab, [dict(o) for o in outputs], [a_lp, b_lp])
    text2, words2, groups = collate.decode_asr(vocab, [dict(o) for o in outputs], return_timestamps="word", return_token_groups=True)
    assert text == text2 and [w["text"] for w in words] == [w["text"] for w in words2] == [" ab", " cd", " ef", " gh", " ij", " kl"]
    assert [w["timestamp"] for w in words] == [w["timestamp"] for w in words2]
    seen = set()
    for w, grp in zip(words, groups):
        assert grp and w["logprob"] == -sum(2.0 ** -i for i in grp)             # exactly the tokens of its group
        members = {i for i in range(n_all) if int(round(-w["logprob"] * 2.0 ** (n_all - 1))) >> (n_all - 1 - i) & 1}
        assert members == set(grp)
        assert not (seen & members)
        seen |= members
    flat = np.concatenate([a_tok, b_tok])
    text_tokens = {i for i in range(n_all) if flat[i] < v.eos}
    assert seen <= text_tokens
    dropped = text_tokens - seen
    assert len(dropped) == len(" ef gh")               # the overlap is decoded twice and kept once: its other copy is in no word
    with pytest.raises(ValueError):
        scored_words(vocab, [dict(o) for o in outputs], [a_lp, b_lp[:-1]])


def test_pack_record_round_trip_with_and_without_scores():
    toks, ts, stride = np.array([1, 2, 300]), np.array([0.5, 1.25, 2.0], np.float32), (30.0, 5.0, 0.0)
    plain = dist.pack_record(7, toks, ts, stride)
    assert plain.shape == (dist.REC_WORDS,) and plain.dtype == np.int32 and dist.REC_WORDS == 6 + 2 * dist.REC_TOKENS
    want = np.zeros(dist.REC_WORDS, np.int32)           # the default record, byte for byte as before the scores existed
    want[0:3] = (7, 3, 3)
    want[3:6] = np.asarray(stride, np.float32).view(np.int32)
    want[6:9] = toks
    want[6 + dist.REC_TOKENS:9 + dist.REC_TOKENS] = ts.view(np.int32)
    assert plain.tobytes() == want.tobytes()
    assert len(dist.unpack_record(plain)) == 4
    lp = np.array([-0.25, 0.0, -17.5], np.float32)
    wide = dist.pack_record(7, toks, ts, stride, lp)
    assert wide.shape == (dist.REC_WORDS_SCORED,) and wide[:dist.REC_WORDS].tobytes() == plain.tobytes()
    idx, t2, ts2, st2, lp2 = dist.unpack_record(wide)
    assert idx == 7 and t2.tolist() == toks.tolist() and ts2.tolist() == ts.tolist() and st2 == stride
    assert lp2.dtype == np.float32 and lp2.tobytes() == lp.tobytes()
    empty = dist.unpack_record(dist.pack_record(3, np.zeros(0, np.int64), np.zeros(0, np.float32), stride, np.zeros(0, np.float32)))
    assert len(empty) == 5 and len(empty[4]) == 0
    with pytest.raises(ValueError):
        dist.pack_record(7, toks, ts, stride, lp[:2])
    # an empty shard keeps the width of the records the other ranks send
    sh = dist.Shard()
    assert sh.all_gather_records(np.zeros((0, dist.REC_WORDS_SCORED), np.int32), 2).shape == (0, dist.REC_WORDS_SCORED)


def test_split_segments_carries_the_values_by_its_index_ranges():
    tb = 1000
    seq = np.array([tb, 5, 6, tb + 10, tb + 10, 7, tb + 20, tb + 20, 8], np.int64)
    n_prompt = 3
    ts = np.arange(n_prompt + len(seq), dtype=np.float32)
    lp = -np.arange(n_prompt + len(seq), dtype=np.float32)
    segs, adv = generation.split_segments(seq, ts, 0.0, tb, 3000, n_prompt, lp)
    plain, adv2 = generation.split_segments(seq, ts, 0.0, tb, 3000, n_prompt)
    assert adv == adv2 and len(segs) == len(plain) == 2
    for s, p in zip(segs, plain):
        assert p.token_logprobs is None and np.array_equal(s.tokens, p.tokens) and s.idxs == p.idxs
        assert s.token_logprobs.dtype == np.float32 and np.array_equal(s.token_logprobs, lp[s.idxs[0]:s.idxs[1]])
        assert len(s.token_logprobs) == len(s.tokens) == len(s.token_timestamps)


def test_return_scores_needs_word_timestamps():
    g, v = syn.tiny_geometry()
    p = object.__new__(CrisperWhisperPipeline)
    p.sampling_seed = None
    p.return_timestamps = True
    p.return_scores = False
    with pytest.raises(ValueError, match="word"):
        p._run_one(np.zeros(16000, np.float32), return_timestamps=True, return_scores=True)
    p.return_scores = True                             # the constructor argument, same refusal
    with pytest.raises(ValueError, match="word"):
        p._run_one(np.zeros(16000, np.float32))


def test_generate_refuses_an_engine_without_the_switch():
    from tests import helpers as Hh
    g, v, W, spec = Hh.tiny_setup()
    eng = Hh.OracleBackedEngine(g, v, W, spec)
    with pytest.raises(ValueError, match="log-probabilities"):
        generation.generate(eng, 1, [3000], language="<|en|>", task="transcribe", return_token_logprobs=True)
