"""Language identification on the device (csrc/langid.hip; cw_detect_language, cw_test_language_probs,
cw_get_transcribe_languages): the kernel against float64 through the comparator of tests/language_refs.py (bound derived there,
faults proven to be rejected in tests/test_language_refs.py), run-to-run and batch independence, the engine entry point against
the logits it consumed and against the route it replaces, and the pipeline's return_language / language_candidates /
detect_language."""
import numpy as np
import pytest

import crisperwhisper_amd as cw
from crisperwhisper_amd import collate, generation, synthetic as syn
from crisperwhisper_amd.engine import Engine
from crisperwhisper_amd.languages import LANGUAGES
from tests import helpers as Hh
from tests import language_refs as R

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "bf16"]
N_LANG = [1, 2, 4, 99, 100, 128]


@pytest.fixture(scope="module")
def tiny():
    return Hh.tiny_setup()


@pytest.fixture(scope="module")
def engines(tiny):
    """Per dtype: the tiny model with its own vocabulary (weights loaded) and the tiny geometry at the vocabulary of large-v3
    (51 866 columns; the kernel does not depend on the model, no weights needed)."""
    g, v, W, spec = tiny
    gl, vl = syn.large_v3_geometry()
    gb, _ = syn.tiny_geometry()
    gb.vocab = gl.vocab
    spec_l = syn.model_spec(gb, vl, n_align=1)
    out = {}
    for dt in DTYPES:
        e = Engine(spec, dtype=dt, max_batch=64)
        e.load_state_dict(W)
        out[dt, "tiny"] = (e, spec)
        out[dt, "large"] = (Engine(spec_l, dtype=dt, max_batch=64), spec_l)
    yield out
    for e, _ in out.values():
        e.close()


def _table(V, n, seed):
    rng = np.random.default_rng(seed)
    ids = V // 2 + rng.permutation(n)
    if n > 1 and not np.any(np.diff(ids) < 0):
        ids = ids[::-1]
    return np.ascontiguousarray(ids, np.int32)


def _rows(V, ids, ns_tok, n_min, seed):
    """The crafted rows, then seeded random ones up to n_min rows: [n][V] f32 (the hook supplies the pad columns itself)."""
    rows = [x[:V] for _, x in R.crafted_rows(V, ids, ns_tok, seed)]
    if len(rows) < n_min:
        rows += list(R.random_rows(V, n_min - len(rows), seed + 1))
    return np.stack(rows)


@pytest.mark.parametrize("nb", [1, 8, 13, 64])
@pytest.mark.parametrize("vocab", ["tiny", "large"])
@pytest.mark.parametrize("dt", DTYPES)
def test_kernel_against_float64(engines, dt, vocab, nb):
    eng, spec = engines[dt, vocab]
    V, ns_tok = spec.vocab_size, spec.no_timestamps_token_id - 1
    assert V == (51866 if vocab == "large" else 1769) and V % 4
    n_rows = 0
    for n in N_LANG:
        ids = _table(V, n, 7 * n + nb)
        rows = _rows(V, ids, ns_tok, nb, 100 * n + nb)
        for lo in range(0, len(rows), nb):
            lg = rows[lo:lo + nb]
            best, prob, ns = eng.test_language_probs(lg, ids, ns_tok)
            assert prob.shape == (len(lg), n)
            R.check_rows(best, prob, ns, lg, ids, V, ns_tok, what=f"{dt} V={V} nb={nb} n_lang={n} rows {lo}..")
            n_rows += len(lg)
        b2, p2, ns2 = eng.test_language_probs(rows[:nb], ids)              # without the no-speech part
        b1, p1, _ = eng.test_language_probs(rows[:nb], ids, ns_tok)
        assert b2.tobytes() == b1.tobytes() and p2.tobytes() == p1.tobytes() and np.isnan(ns2).all()
    assert n_rows >= len(N_LANG) * max(nb, 6)


@pytest.mark.parametrize("vocab", ["tiny", "large"])
@pytest.mark.parametrize("dt", DTYPES)
def test_a_row_does_not_depend_on_its_index_its_batch_or_the_run(engines, dt, vocab):
    eng, spec = engines[dt, vocab]
    V, ns_tok = spec.vocab_size, spec.no_timestamps_token_id - 1
    ids = _table(V, 100, 3)
    rows = _rows(V, ids, ns_tok, 8, 55)[:8]

    def run(lg):
        b, p, s = eng.test_language_probs(lg, ids, ns_tok)
        return [(b[r].tobytes(), p[r].tobytes(), s[r].tobytes()) for r in range(len(lg))]
    base = run(rows)
    assert run(rows) == base                                            # run to run
    assert run(rows[::-1])[::-1] == base                                # another index
    assert [run(rows[r:r + 1])[0] for r in range(8)] == base            # alone
    big = R.random_rows(V, 64, 77)
    big[37], big[63], big[0] = rows[2], rows[5], rows[7]
    got = run(big)
    assert (got[37], got[63], got[0]) == (base[2], base[5], base[7])    # inside a full batch


def test_hook_refuses_bad_tables(engines):
    eng, spec = engines["f32", "tiny"]
    lg = np.zeros((2, spec.vocab_size), np.float32)
    for bad in ([], [5, 5], [spec.vocab_size], [-1], list(range(129))):
        with pytest.raises(Exception):
            eng.test_language_probs(lg, bad)
    eng.mel([syn.synth_audio(1, 16000, "noise")])
    eng.encode([0], [0], [3000])
    for bad in ([], [5, 5], [spec.vocab_size], list(range(129))):
        with pytest.raises(Exception):
            eng.detect_language(1, bad)
    with pytest.raises(Exception):
        eng.detect_language(2)                                          # one window encoded


def _clips(nb, secs=2):
    kinds = ("noise", "chirp", "mixed")
    return [syn.synth_audio(100 + b, secs * 16000, kinds[b % 3]) for b in range(nb)]


@pytest.mark.parametrize("nb", [3, 12])
@pytest.mark.parametrize("dt", DTYPES)
def test_engine_detect_language(tiny, engines, dt, nb):
    """After encode: the results against float64 on the logits read back after the call, the no-speech probability against
    cw_no_speech_probs, the position-0 logits bit for bit those of the route this replaces (decode of one step on
    <|startoftranscript|>; 12 rows: the short-history attention of 9 rows and more), and that route's languages."""
    g, v, W, spec = tiny
    eng, _ = engines[dt, "tiny"]
    V, ns_tok = spec.vocab_size, spec.no_timestamps_token_id - 1
    lang_ids = np.array(sorted(spec.lang_to_id.values()), np.int32)
    eng.mel(_clips(nb))
    eng.encode(list(range(nb)), [0] * nb, [3000] * nb)
    eng.decode(np.full((nb, 1), spec.decoder_start_token_id, np.int32), max_length=2)      # the old route
    lg_old = eng.last_logits(nb)
    old_ids = lang_ids[np.argmax(lg_old[:, lang_ids], axis=-1)]
    ids, prob, ns = eng.detect_language(nb)
    lg = eng.last_logits(nb)
    assert lg.tobytes() == lg_old.tobytes()
    assert ids.tolist() == old_ids.tolist()
    assert ids.dtype == np.int32 and prob.shape == (nb, len(lang_ids)) and ns.shape == (nb,)
    R.check_rows(ids, prob, ns, lg, lang_ids, V, ns_tok, what=f"{dt} detect_language nb={nb}")
    again = eng.detect_language(nb)
    assert again[0].tobytes() == ids.tobytes() and again[1].tobytes() == prob.tobytes() and again[2].tobytes() == ns.tobytes()
    if nb <= 8:             # (cw_no_speech_probs keeps its own forward: from 9 rows on that is the long-history attention)
        nsp = eng.no_speech_probs(nb, spec.decoder_start_token_id)
        for b in range(nb):
            bd = R.ns_bound(lg[b], V, ns_tok) + R.U * float(nsp[b])      # its float64 result, rounded to f32 once
            print(f"row {b}: kernel {ns[b]!r} host {nsp[b]!r} bound {bd:.3e}")
            assert abs(float(ns[b]) - float(nsp[b])) <= bd
    # a restricted table: only those ids, and their own softmax
    sub = lang_ids[[2, 0]]
    ids2, prob2, ns2 = eng.detect_language(nb, sub, no_speech=False)
    assert ns2 is None and set(ids2.tolist()) <= set(sub.tolist())
    R.check_rows(ids2, prob2, None, eng.last_logits(nb), sub, V, -1, what=f"{dt} two candidates")
    assert generation.detect_language(eng, nb).tolist() == old_ids.tolist()


# ---- pipeline -------------------------------------------------------------------------------------------------------------
W_SEED = 24      # weights with which the windows of RECORDING below are detected as english, german, spanish (asserted)


@pytest.fixture(scope="module")
def tiny_varied():
    return Hh.tiny_setup(seed=W_SEED)


@pytest.fixture(scope="module")
def pipe(tiny_varied):
    g, v, W, spec = tiny_varied
    p = cw.pipeline("automatic-speech-recognition", model=cw.ModelBundle(spec, W), tokenizer=collate.Vocabulary.from_synthetic(v),
                    chunk_length_s=30, batch_size=2, return_timestamps="word", torch_dtype="float32", device="cuda:0")
    yield p
    for e in p.engines:
        e.close()


def _recording():
    """70 s: 25 s chirp, 20 s tone bursts in noise with a silent stretch, 25 s silence -- three strided 30 s windows."""
    return np.concatenate([syn.synth_audio(30, 25 * 16000, "chirp"), syn.synth_audio(31, 20 * 16000, "mixed"),
                           np.zeros(25 * 16000, np.float32)])


GK = {"num_beams": 1, "max_new_tokens": 16}


def _strip(chunks, *keys):
    return [{k: c[k] for k in c if k not in keys} for c in chunks]


def _same(a, b):
    """chunk lists equal, NaN == NaN"""
    return repr(a) == repr(b)


def _expected(pipe, x, mode="word", gk=GK, seed=0, language_candidates=None):
    """What the strided call has to return with return_language: generation.generate on the same windows in the pipeline's own
    batches, every window's tokens prefixed with ITS entry of out["languages"] (and a 0.0 timestamp), through the collator
    (held against transformers in tests/test_language_host.py).  -> (text, chunks, the windows' language tokens)."""
    from crisperwhisper_amd import audio
    wins = audio.chunk_windows(len(x), 480000, 80000, 80000)
    outs, langs = [], []
    for b0 in range(0, len(wins), pipe.batch_size):
        idxs = list(range(b0, min(len(wins), b0 + pipe.batch_size)))
        _, nf = pipe.engine.mel([x[wins[i][0]: wins[i][0] + wins[i][1]] for i in idxs])
        o = generation.generate(pipe.engine, len(idxs), nf, language=gk.get("language"), task=gk.get("task"),
                                max_new_tokens=gk.get("max_new_tokens"), num_beams=gk.get("num_beams", 1),
                                prompt_ids=gk.get("prompt_ids"), temperature=gk.get("temperature"),
                                compression_ratio_threshold=gk.get("compression_ratio_threshold"), sampling_seed=seed,
                                item_ids=idxs, language_candidates=language_candidates)
        for k, i in enumerate(idxs):
            n = len(o["token_timestamps"][k])
            lang = int(o["languages"][k])
            langs.append(lang)
            outs.append({"tokens": np.concatenate([[lang], o["sequences"][k][:n]]),
                         "token_timestamps": np.concatenate([np.zeros(1, np.float32), o["token_timestamps"][k]]),
                         "stride": tuple(t / 16000 for t in wins[i][2])})
    text, chunks = collate.decode_asr(pipe.vocab, outs, return_timestamps=mode, return_language=True)
    return text, chunks, langs


@pytest.mark.parametrize("mode", ["word", True])
def test_return_language_strided_long_form(tiny_varied, pipe, mode):
    """Three strided windows detected as three different languages: chunk for chunk -- text, timestamp, language -- what the
    collator makes of every window's tokens behind that window's own language token; text and timestamps equal the call
    without return_language."""
    g, v, W, spec = tiny_varied
    x = _recording()
    plain = pipe(x, return_timestamps=mode, generate_kwargs=GK)
    got = pipe(x, return_timestamps=mode, generate_kwargs=GK, return_language=True)
    text, chunks, langs = _expected(pipe, x, mode)
    assert langs == [v.lang_id("en"), v.lang_id("de"), v.lang_id("es")]      # not one language, and the two of a batch differ
    assert got["text"] == text and got["chunks"] == chunks and chunks
    # (a segment merged across a seam takes the later window's language, as in transformers: not every window need show)
    assert len({c["language"] for c in chunks}) >= 2 and chunks[0]["language"] == "english" and chunks[-1]["language"] == "spanish"
    assert set(plain["chunks"][0]) == {"text", "timestamp"}
    assert got["text"] == plain["text"] and _strip(got["chunks"], "language") == plain["chunks"]


def test_return_language_keeps_every_per_token_array_aligned(tiny_varied, pipe):
    g, v, W, spec = tiny_varied
    x = _recording()
    kw = dict(generate_kwargs=GK, return_scores=True, top_logprobs=2, return_alignment_scores=True)
    plain = pipe(x, **kw)
    got = pipe(x, return_language=True, **kw)
    text, chunks, langs = _expected(pipe, x)
    assert len(set(langs)) == 3
    assert got["text"] == plain["text"] == text and got["chunks"]
    assert _same(_strip(got["chunks"], "language"), plain["chunks"])     # logprob, tokens, alignment_score, alignment_spread
    assert [{k: c[k] for k in ("text", "timestamp", "language")} for c in got["chunks"]] == chunks


def _modes(v):
    return {"beam": {"num_beams": 3, "max_new_tokens": 12},
            "forced": {"num_beams": 1, "max_new_tokens": 12, "language": "de"},
            "fallback": {"num_beams": 1, "max_new_tokens": 12, "temperature": (0.0, 0.6), "compression_ratio_threshold": 1.2},
            "prompted": {"num_beams": 1, "max_new_tokens": 12, "prompt_ids": [v.startofprev, ord(" "), ord("D"), ord("r"), ord(".")]}}


@pytest.mark.parametrize("name", ["beam", "forced", "fallback", "prompted"])
def test_return_language_in_the_other_decoding_modes(tiny_varied, pipe, name):
    """Beam search, a forced language, sampling with fallback, prompt_ids (the language token leads the window's tokens, the
    prompt is never among them): every chunk as the collator makes it behind each window's own language, nothing else moves."""
    g, v, W, spec = tiny_varied
    gk = _modes(v)[name]
    x = _recording()
    plain = pipe(x, generate_kwargs=gk, sampling_seed=7)
    got = pipe(x, generate_kwargs=gk, sampling_seed=7, return_language=True)
    text, chunks, langs = _expected(pipe, x, gk=gk, seed=7)
    assert got["text"] == text and got["chunks"] == chunks and chunks
    assert got["text"] == plain["text"] and _strip(got["chunks"], "language") == plain["chunks"]
    if name == "forced":
        assert langs == [v.lang_id("de")] * 3 and all(c["language"] == "german" for c in got["chunks"])
    else:
        assert len(set(langs)) == 3
    if name == "prompted":                                               # ... together with the per-token arrays
        kw = dict(generate_kwargs=gk, return_scores=True, top_logprobs=2, return_alignment_scores=True)
        a, b = pipe(x, **kw), pipe(x, return_language=True, **kw)
        assert _same(_strip(b["chunks"], "language"), a["chunks"])
        assert [{k: c[k] for k in ("text", "timestamp", "language")} for c in b["chunks"]] == chunks


def test_forced_chinese_splits_per_character_like_the_collator(tiny_varied, pipe):
    """A language written without spaces changes word splitting, as in transformers: the pipeline's chunks equal the collator's
    on the language-prefixed stream (held against transformers in tests/test_language_host.py)."""
    g, v, W, spec = tiny_varied
    x = syn.synth_audio(3, 20 * 16000, "mixed")
    got = pipe(x, generate_kwargs=dict(GK, language="zh"), return_language=True)
    _, nf = pipe.engine.mel([x])
    o = generation.generate(pipe.engine, 1, nf, language="zh", num_beams=1, max_new_tokens=16)
    assert o["languages"].tolist() == [v.lang_id("zh")] and np.isnan(o["language_probs"]).all()
    n = len(o["token_timestamps"][0])
    toks = np.concatenate([[v.lang_id("zh")], o["sequences"][0][:n]])
    ts = np.concatenate([np.zeros(1, np.float32), o["token_timestamps"][0]])
    text, words = collate.decode_asr(pipe.vocab, [{"tokens": toks, "token_timestamps": ts, "stride": (20.0, 0.0, 0.0)}],
                                     return_language=True)
    assert got["text"] == text and got["chunks"] == words and words
    assert all(c["language"] == "chinese" for c in got["chunks"])
    plain = pipe(x, generate_kwargs=dict(GK, language="zh"))
    assert plain["text"] == got["text"] and len(got["chunks"]) >= len(plain["chunks"])


def test_language_candidates_native_and_host_loops_agree(tiny_varied, pipe):
    g, v, W, spec = tiny_varied
    eng = pipe.engine
    clips = _clips(2, secs=8)
    de_es = sorted([v.lang_id("de"), v.lang_id("es")])
    outs = []
    for native in (True, False):
        _, nf = eng.mel(clips)
        outs.append(generation.generate(eng, 2, nf, language=None, task="transcribe", num_beams=1, max_new_tokens=12,
                                        native=native, language_candidates=["de", "es"]))
    a, b = outs
    assert set(a["languages"].tolist()) <= set(de_es)
    assert a["languages"].tolist() == b["languages"].tolist()            # cw_get_transcribe_languages == the Python seek loop
    assert a["language_probs"].tobytes() == b["language_probs"].tobytes() and np.all(a["language_probs"] >= 0.5)
    assert np.array_equal(a["sequences"], b["sequences"])
    x = _recording()
    got = pipe(x, generate_kwargs=GK, language_candidates=["de", "es"], return_language=True)
    text, chunks, langs = _expected(pipe, x, language_candidates=["de", "es"])
    assert set(langs) == set(de_es)                                      # both occur, nothing else does
    assert got["text"] == text and got["chunks"] == chunks and chunks    # ... each at the words of its own window
    # cw_transcribe itself: an id listed twice in cfg->lang_ids counts once, as in the host loop the kernel replaced; a forced
    # token that is none of cfg->lang_ids is reported as no language
    _, nf = eng.mel(clips)
    kw = dict(sot=spec.decoder_start_token_id, task_token=v.transcribe, max_new_tokens=6, max_length=spec.max_length)
    t1 = eng.transcribe(2, nf, lang_ids=de_es, **kw)
    l1 = eng.transcribe_languages(2)
    t2 = eng.transcribe(2, nf, lang_ids=[de_es[1], de_es[0], de_es[1]], **kw)
    l2 = eng.transcribe_languages(2)
    assert l1[0].tolist() == l2[0].tolist() == a["languages"].tolist() and l1[1].tobytes() == l2[1].tobytes()
    assert all(np.array_equal(p, q) for p, q in zip(t1[0], t2[0]))
    eng.transcribe(2, nf, language_token=v.transcribe, lang_ids=sorted(spec.lang_to_id.values()), **kw)
    ltok, lprob = eng.transcribe_languages(2)
    assert ltok.tolist() == [-1, -1] and np.isnan(lprob).all()
    eng.transcribe(2, nf, language_token=v.lang_id("es"), lang_ids=sorted(spec.lang_to_id.values()), **kw)
    assert eng.transcribe_languages(2)[0].tolist() == [v.lang_id("es")] * 2
    _, nf = eng.mel(clips)
    free = generation.generate(eng, 2, nf, language=None, task="transcribe", num_beams=1, max_new_tokens=12)
    assert free["language_probs"].dtype == np.float32 and np.all(free["language_probs"] > 0.25 - 1e-6)   # the winner of four


def test_pipe_detect_language(tiny_varied, pipe):
    g, v, W, spec = tiny_varied
    short, long_ = syn.synth_audio(11, 5 * 16000, "chirp"), syn.synth_audio(12, 70 * 16000, "mixed")
    one = pipe.detect_language(short)
    assert set(one) == {"language", "code", "token_id", "probability", "no_speech_prob", "probabilities", "windows"}
    assert list(one["probabilities"]) == ["en", "zh", "de", "es"] and len(one["windows"]) == 1
    assert one["windows"][0]["timestamp"] == (0.0, 5.0)
    assert {k: one[k] for k in one if k != "windows"} == {k: one["windows"][0][k] for k in one if k != "windows"}
    assert one["language"] == LANGUAGES[one["code"]] and one["token_id"] == v.lang_id(one["code"])
    assert one["probability"] == max(one["probabilities"].values()) and 0.0 <= one["no_speech_prob"] <= 1.0
    lg = pipe.engine.last_logits(1)[0]                                   # the logits that call consumed
    ids = np.array(sorted(spec.lang_to_id.values()))
    assert abs(sum(one["probabilities"].values()) - 1.0) <= R.prob_bound(lg, ids).sum()
    both = pipe.detect_language([short, long_])
    assert {k: both[0][k] for k in both[0]} == one                       # a row does not depend on its batch
    many = both[1]
    assert [w["timestamp"] for w in many["windows"]] == [(0.0, 30.0), (30.0, 60.0), (60.0, 70.0)]
    for w in many["windows"] + [many]:
        assert abs(sum(w["probabilities"].values()) - 1.0) <= R.sum_bound(4)
    mean = np.mean(np.stack([[w["probabilities"][c] for c in ("en", "zh", "de", "es")] for w in many["windows"]]), axis=0)
    assert [many["probabilities"][c] for c in ("en", "zh", "de", "es")] == mean.tolist()
    assert many["no_speech_prob"] == float(np.mean([w["no_speech_prob"] for w in many["windows"]]))
    assert many["probability"] == mean.max() and many["code"] == ("en", "zh", "de", "es")[int(np.argmax(mean))]
    only = pipe.detect_language(long_, candidates=["german"])
    assert only["code"] == "de" and only["probability"] == 1.0 and all(w["probability"] == 1.0 for w in only["windows"])
    assert only["no_speech_prob"] == many["no_speech_prob"]
    with pytest.raises(ValueError):
        pipe.detect_language(short, candidates=["de", "german"])
    with pytest.raises(ValueError):
        pipe.detect_language(short, candidates=[])
