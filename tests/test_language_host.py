"""Host side of language identification (no GPU): the C ABI surface, the collator's language bookkeeping against the installed
transformers tokenizer, generation.generate's "languages" over the oracle-backed engine, and the argument refusals."""
import os
import re

import numpy as np
import pytest

from crisperwhisper_amd import _native, audio, collate, generation, synthetic as syn
from crisperwhisper_amd.languages import LANGUAGES
from oracle import generate as OG
from tests import helpers as Hh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"cw_detect_language": 8, "cw_test_language_probs": 9, "cw_get_transcribe_languages": 4, "cw_collate_get_languages": 2}


def test_symbols_prototypes_and_abi_version():
    hdr = open(os.path.join(ROOT, "include", "crisperwhisper.h")).read()
    lib = _native.load()
    assert re.search(r"#define\s+CW_LANG_IDS_MAX\s+128\b", hdr) and generation.LANG_IDS_MAX == 128
    for name, n_args in NEW.items():
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/crisperwhisper.h"
        args = [a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()]
        assert len(args) == n_args, (name, args)
        assert hasattr(lib, name), f"{name} is not exported"
        res, sig = _native._SIGS[name]
        assert res is _native._I and len(sig) == n_args, (name, sig)
    assert lib.cw_abi_version() == 1


# ---- collator against transformers ------------------------------------------------------------------------------------------
def _hf_decode(tok, outs, mode):
    import torch
    hf_in = []
    for o in outs:
        d = {"tokens": torch.tensor(np.asarray(o["tokens"]))[None], "stride": o["stride"]}
        if mode == "word":
            d["token_timestamps"] = torch.tensor(np.asarray(o["token_timestamps"], np.float32))[None]
        hf_in.append(d)
    return tok._decode_asr(hf_in, return_timestamps=mode, return_language=True, time_precision=0.02)


def _check_against_hf(tok, pv, outs, what):
    """text, timestamps and language equal, chunk for chunk, in word and in segment mode; returns the word chunks"""
    words = None
    for mode in ("word", True):
        text, opt = _hf_decode(tok, outs, mode)
        got = collate.decode_asr(pv, [dict(o) for o in outs], return_timestamps=mode, return_language=True)
        assert got[0] == text, (what, mode)
        assert len(got[1]) == len(opt["chunks"]), (what, mode, len(got[1]), len(opt["chunks"]))
        for k, (a, b) in enumerate(zip(got[1], opt["chunks"])):
            assert set(a) == {"text", "timestamp", "language"}
            assert (a["text"], tuple(a["timestamp"]), a["language"]) == (b["text"], tuple(b["timestamp"]), b["language"]), (what, mode, k, a, b)
        # the language is bookkeeping only: the other fields are those of the call without it
        plain = collate.decode_asr(pv, [dict(o) for o in outs], return_timestamps=mode)
        assert plain[0] == got[0] and plain[1] == [{"text": c["text"], "timestamp": c["timestamp"]} for c in got[1]]
        assert all(set(c) == {"text", "timestamp"} for c in plain[1])
        if mode == "word":
            words = got[1]
    return words


def _stream(v, lang, segs, ts_step=0.3):
    """One window: [<|lang|>] + for every (t0, bytes, t1): <|t0|> text <|t1|> (t1 None: left open); token timestamps with a 0.0
    in front for the language token."""
    tb = v.timestamp_begin
    toks = [] if lang is None else [v.lang_id(lang)]
    for t0, body, t1 in segs:
        if t0 is not None:
            toks.append(tb + t0)
        toks += list(body)
        if t1 is not None:
            toks.append(tb + t1)
    ts = np.round(np.arange(len(toks)) * ts_step, 2).astype(np.float32)
    if lang is not None:
        ts[0] = 0.0
    return toks, ts


def test_collator_languages_match_transformers_on_hand_built_streams():
    pytest.importorskip("transformers")
    from tests.golden import hf_synth as H
    g, v = syn.tiny_geometry()
    tok, pv = H.build_tokenizer(v), collate.Vocabulary.from_synthetic(v)
    A, B, C = list(b" ab cd."), list(b" ef, gh"), list("你好吗".encode())
    seam = list(b" seam words here")

    def outs_of(windows):
        n = len(windows)
        return [{"tokens": np.array(t), "token_timestamps": ts, "stride": (30.0, 0.0 if k == 0 else 5.0, 0.0 if k == n - 1 else 5.0)}
                for k, (t, ts) in enumerate(windows)]

    # en -> de -> zh, every segment closed inside its window; the last language is written without spaces
    outs = outs_of([_stream(v, "en", [(0, A, 400), (400, B, 900)]), _stream(v, "de", [(300, B, 800), (800, A, 1100)]),
                    _stream(v, "zh", [(300, C, 700), (700, C + A, 1400)])])
    words = _check_against_hf(tok, pv, outs, "en-de-zh")
    assert [w["language"] for w in words][0] == "english" and words[-1]["language"] == "chinese"
    assert {"english", "german", "chinese"} == {w["language"] for w in words}
    assert sum(w["language"] == "chinese" for w in words) >= 6          # split per character
    # a segment left open in the English window and closed in the German one: merged across the seam, it takes the later
    # window's language (its words are collated when it is flushed)
    outs = outs_of([_stream(v, "en", [(0, A, 300), (350, B + seam, None)]), _stream(v, "de", [(None, seam + A, 600), (600, B, 900)])])
    words = _check_against_hf(tok, pv, outs, "seam")
    merged = [w for w in words if "ef" in w["text"] or "seam" in w["text"]]
    assert merged and all(w["language"] == "german" for w in merged)
    assert words[0]["language"] == "english"
    # no language token anywhere: None throughout
    outs = outs_of([_stream(v, None, [(0, A, 400)]), _stream(v, None, [(300, B, 800)])])
    words = _check_against_hf(tok, pv, outs, "no language")
    assert words and all(w["language"] is None for w in words)
    # one window without strides, language in front
    t, ts = _stream(v, "es", [(0, A + B, 500)])
    words = _check_against_hf(tok, pv, [{"tokens": np.array(t), "token_timestamps": ts, "stride": (30.0, 0.0, 0.0)}], "single")
    assert all(w["language"] == "spanish" for w in words)


def test_collator_languages_match_transformers_on_random_streams():
    pytest.importorskip("transformers")
    from tests.golden import hf_synth as H
    g, v = syn.tiny_geometry()
    tok, pv = H.build_tokenizer(v), collate.Vocabulary.from_synthetic(v)
    rng = np.random.default_rng(31)
    tb = v.timestamp_begin
    alphabet = [32, 32, 46, 44, 39, 40, 45, 34, 65, 66, 97, 98, 0xc3, 0xa9, 0xe4, 0xbd, 0xa0, 0xe5, 0xa5, 0xbd]
    seen = set()
    for trial in range(30):
        outs = []
        n_chunks = int(rng.integers(1, 4))
        common = rng.choice(alphabet, size=6).tolist()
        langs = [("en", "de", "zh", None)[int(rng.integers(0, 4))] for _ in range(n_chunks)]
        for c in range(n_chunks):
            toks, t = ([] if langs[c] is None else [v.lang_id(langs[c])]), 0
            for _ in range(int(rng.integers(1, 4))):
                t0 = t + int(rng.integers(0, 300)); t1 = t0 + int(rng.integers(1, 400)); t = min(t1, 1500)
                body = rng.choice(alphabet, size=int(rng.integers(1, 10))).tolist()
                if rng.random() < 0.5:
                    body = common + body          # overlapping text across chunk seams
                toks += [tb + min(t0, 1500)] + body + [tb + t]
            if rng.random() < 0.3:
                toks = toks[:-1]                  # left open: closed by a later window, or never
            ts = np.round(np.sort(rng.random(len(toks)) * 30), 2).astype(np.float32)
            if langs[c] is not None:
                ts[0] = 0.0
            outs.append({"tokens": np.array(toks), "token_timestamps": ts,
                         "stride": (30.0, 0.0 if c == 0 else 5.0, 0.0 if c == n_chunks - 1 else 5.0)})
        words = _check_against_hf(tok, pv, outs, f"trial {trial}")
        seen |= {w["language"] for w in words}
    assert seen == {"english", "german", "chinese", None}


# ---- generation.generate over the oracle-backed engine ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["noise40_b2_autolang", "mixed20_b1_autolang_notask", "chirp12_b1_n24"])
def test_generate_reports_the_language_of_every_item(name):
    """Auto-detection: the token the oracle's own generate puts into the prompt; a forced language: that token, NaN probability."""
    g, v, W, spec = Hh.tiny_setup()
    meta = Hh.gold_json("e2e_golden.json")[name]
    x = syn.synth_audio(meta["seed"], int(round(meta["secs"] * 16000)), meta["kind"])
    eng = Hh.OracleBackedEngine(g, v, W, spec)
    windows = audio.chunk_windows(len(x), 480000, 80000, 80000)
    kw = {"language": "<|en|>", "task": "transcribe", **meta["extra"]}
    for b0 in range(0, len(windows), meta["batch_size"]):
        batch = windows[b0:b0 + meta["batch_size"]]
        feats, nf = eng.mel([x[s:s + n] for s, n, _, _ in batch], return_features=True)
        out = generation.generate(eng, len(batch), nf, language=kw["language"], task=kw["task"],
                                  max_new_tokens=kw.get("max_new_tokens"), min_new_tokens=kw.get("min_new_tokens"))
        assert out["languages"].dtype == np.int64 and out["languages"].shape == (len(batch),)
        assert out["language_probs"].dtype == np.float32 and out["language_probs"].shape == (len(batch),)
        if kw["language"] is None:
            want = OG.detect_language(eng.model, eng.ospec, feats)
            assert out["languages"].tolist() == [int(t) for t in want]
            assert np.all((out["language_probs"] >= 0.25 - 1e-6) & (out["language_probs"] <= 1.0))    # the winner of four
        else:
            assert out["languages"].tolist() == [v.lang_id("en")] * len(batch) and np.isnan(out["language_probs"]).all()


def test_language_candidates_restrict_detection_and_are_checked():
    g, v, W, spec = Hh.tiny_setup()
    eng = Hh.OracleBackedEngine(g, v, W, spec)
    _, nf = eng.mel([syn.synth_audio(8, 40000, "noise"), syn.synth_audio(9, 40000, "mixed")])
    free = generation.generate(eng, 2, nf, language=None, task="transcribe", max_new_tokens=6)
    others = [c for c in ("en", "zh", "de", "es") if v.lang_id(c) not in free["languages"].tolist()]
    out = generation.generate(eng, 2, nf, language=None, task="transcribe", max_new_tokens=6, language_candidates=others[:2])
    assert set(out["languages"].tolist()) <= {v.lang_id(c) for c in others[:2]}
    assert np.all(out["language_probs"] >= 0.5 - 1e-6)                   # the winner of two
    one = generation.generate(eng, 2, nf, language=None, task="transcribe", max_new_tokens=6, language_candidates=["German"])
    assert one["languages"].tolist() == [v.lang_id("de")] * 2 and one["language_probs"].tolist() == [1.0, 1.0]
    assert generation.check_language_candidates(spec, ["es", "<|en|>", "german"]) == sorted(v.lang_id(c) for c in ("en", "de", "es"))
    assert generation.check_language_candidates(spec, None) is None
    for bad in ([], ["de", "german"], ["xx"], "de", [3], ["de", "<|de|>"]):
        with pytest.raises(ValueError):
            generation.generate(eng, 2, nf, language=None, task="transcribe", language_candidates=bad)
    with pytest.raises(ValueError):                                      # together with an explicit language
        generation.generate(eng, 2, nf, language="en", task="transcribe", language_candidates=["de"])
    import dataclasses
    with pytest.raises(ValueError):                                      # an English-only checkpoint has nothing to detect
        generation.check_language_candidates(dataclasses.replace(spec, lang_to_id={}), ["en"])


def test_return_language_off_leaves_the_chunk_keys_alone():
    g, v = syn.tiny_geometry()
    pv = collate.Vocabulary.from_synthetic(v)
    t, ts = _stream(v, "de", [(0, list(b" ab cd"), 400)])
    outs = [{"tokens": np.array(t), "token_timestamps": ts, "stride": (30.0, 0.0, 0.0)}]
    for mode in ("word", True):
        text, chunks = collate.decode_asr(pv, outs, return_timestamps=mode)
        assert chunks and all(set(c) == {"text", "timestamp"} for c in chunks)
        text2, chunks2, groups = collate.decode_asr(pv, outs, return_timestamps=mode, return_token_groups=True, return_language=True)
        assert text2 == text and all(c["language"] == LANGUAGES["de"] for c in chunks2)
        assert all(0 not in g_ for g_ in groups)                         # the language token belongs to no chunk


# ---- the pipeline over a scripted engine: strided windows, every per-token array, the sharded gather -----------------------
def _same(a, b):
    return repr(a) == repr(b)                       # NaN == NaN


@pytest.mark.parametrize("extras", [{}, {"return_scores": True, "top_logprobs": 2, "return_alignment_scores": True}])
def test_pipeline_return_language_strided_and_sharded(extras):
    """Three strided windows detected as en / de / es: every word names the language in force, text and timestamps and every
    per-token quantity equal the call without return_language, the records keep their widths, and 2 and 4 ranks gather the same."""
    from crisperwhisper_amd import dist
    from tests import language_doubles as D
    g, v, W, spec = Hh.tiny_setup()
    gk = {"num_beams": 1, "task": "transcribe"}
    plain = D.make_pipe(spec, v, D.LangScriptedEngine(spec, v, [0, 1, 2]))(D.PCM, generate_kwargs=gk, **extras)
    got = D.make_pipe(spec, v, D.LangScriptedEngine(spec, v, [0, 1, 2]))(D.PCM, generate_kwargs=gk, return_language=True, **extras)
    assert got["text"] == plain["text"] and got["chunks"]
    assert _same([{k: c[k] for k in c if k != "language"} for c in got["chunks"]], plain["chunks"])
    assert all("language" not in c for c in plain["chunks"])
    langs = [c["language"] for c in got["chunks"]]
    # every window's own language arrives at its words (a segment merged across a seam takes the later window's, as in transformers)
    assert langs[0] == "english" and langs[-1] == "spanish" and set(langs) == {"english", "german", "spanish"}
    assert langs == sorted(langs, key=["english", "german", "spanish"].index)          # in audio order
    # the collator on the language-prefixed stream says the same (held against transformers above)
    sc = D.script(v)
    outs = [{"tokens": np.concatenate([[v.lang_id(l)], s[0]]), "token_timestamps": np.concatenate([[0.0], s[1]]).astype(np.float32),
             "stride": st} for s, l, st in zip(sc, D.LANGS, D.STRIDES)]
    text, words, groups = collate.decode_asr(collate.Vocabulary.from_synthetic(v), outs, return_language=True, return_token_groups=True)
    assert text == got["text"] and words == [{k: c[k] for k in ("text", "timestamp", "language")} for c in got["chunks"]]
    flat = np.concatenate([o["tokens"] for o in outs])
    used = {int(i) for grp in groups for i in grp}
    assert {i for i in range(len(flat)) if flat[i] < v.eos} - used          # the overlaps are decoded twice and kept once
    if extras:      # the values name their tokens: a word sums exactly its own group, shifted by the language tokens in front
        lp = np.concatenate([np.concatenate([[np.nan], s[2]]) for s in sc]).astype(np.float64)
        mass = np.concatenate([np.concatenate([[np.nan], s[3]]) for s in sc]).astype(np.float64)
        for c, grp in zip(got["chunks"], groups):
            assert c["logprob"] == float(np.sum(lp[grp])) and c["alignment_score"] == float(np.mean(mass[grp]))
            assert [t["id"] for t in c["tokens"]] == [int(flat[i]) for i in grp]
    width = dist.REC_WORDS if not extras else dist.rec_words_top(2) + dist.REC_ALIGN_WORDS
    for world in (2, 4):
        bounds, sent = dist.shard_bounds(3, world), []
        for r, (lo, hi) in enumerate(bounds):
            sh = D.CaptureShard(r, world)
            with pytest.raises(D.Captured):
                D.make_pipe(spec, v, D.LangScriptedEngine(spec, v, range(lo, hi)), shard=sh)(D.PCM, generate_kwargs=gk, return_language=True, **extras)
            assert sh.sent.shape == (hi - lo, width)                                  # the record layouts are unchanged
            sent.append(sh.sent)
        lo, hi = bounds[0]
        again = D.make_pipe(spec, v, D.LangScriptedEngine(spec, v, range(lo, hi)), shard=D.ReplayShard(sent, world))(
            D.PCM, generate_kwargs=gk, return_language=True, **extras)
        assert _same(again, got)
    # batches of two windows: the k-th language of a batch goes to the k-th window of the batch
    two = D.make_pipe(spec, v, D.LangScriptedEngine(spec, v, [0, 1, 2]), batch_size=2)(D.PCM, generate_kwargs=gk, return_language=True, **extras)
    assert _same(two, got)


def test_pipeline_language_arguments_are_checked_before_any_audio_work():
    from tests import language_doubles as D
    g, v, W, spec = Hh.tiny_setup()

    class NoAudio(D.LangScriptedEngine):
        def mel(self, clips):
            raise AssertionError("audio work started")
    pipe = D.make_pipe(spec, v, NoAudio(spec, v, [0, 1, 2]))
    for kw in ({"language_candidates": []}, {"language_candidates": ["de", "german"]}, {"language_candidates": ["xx"]},
               {"language_candidates": "de"},
               {"language_candidates": ["de"], "generate_kwargs": {"num_beams": 1, "language": "en"}}):
        with pytest.raises(ValueError):
            pipe(D.PCM, **{"generate_kwargs": {"num_beams": 1}, **kw})
    with pytest.raises(ValueError):                           # not a generate_kwargs key: the pinned list is untouched
        pipe(D.PCM, generate_kwargs={"num_beams": 1, "language_candidates": ["de"]})
    with pytest.raises(ValueError):
        pipe.detect_language(D.PCM, candidates=["de", "<|de|>"])
