"""Temperature fallback end to end on the device against what transformers computes deterministically
(tests/golden/gen_golden_fallback.py): every temperature-0 decode of a window -- tokens, compression ratio, average
log-probability, no-speech probability, decision -- and the words of the windows that never fall back; for the windows that
do, the properties of the kept result (it satisfies the thresholds or comes from the last temperature, its tokens are the
float64 argmax of the perturbed scores of the decode that produced them, its timestamps are that decode's); and through the
pipeline, independence of the batch size and dependence on the seed.

Tolerances: the quantities as tests/test_gpu_e2e.py::test_logprob_and_no_speech_thresholds_vs_transformers compares them
(no-speech probability 1e-4 relative, average log-probability 2e-3), the compression ratio exactly (same tokens, same zlib), words
within 20 ms, timestamps against forced alignment of the same tokens within the 0.02 s + 1e-6 tests/test_gpu_align.py asserts
between its two forward paths."""
import numpy as np
import pytest

import crisperwhisper_amd as cw
from crisperwhisper_amd import collate, generation
from tests import helpers as Hh
from tests import sampling_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tiny():
    return Hh.tiny_setup()


@pytest.fixture(scope="module")
def gold():
    return Hh.gold_json("e2e_fallback_golden.json")


def _pipe(tiny, batch_size, **kw):
    g, v, W, spec = tiny
    kw.setdefault("sampling_seed", 0)
    return cw.pipeline("automatic-speech-recognition", model=cw.ModelBundle(spec, W), tokenizer=collate.Vocabulary.from_synthetic(v),
                       chunk_length_s=30, batch_size=batch_size, return_timestamps="word", torch_dtype="float32",
                       device="cuda:0", num_beams=1, **kw)


def _gk(gold):
    gk = dict(gold["generate_kwargs"])
    gk["temperature"] = tuple(gk["temperature"])
    return gk


def test_temperature_zero_decisions_and_kept_windows_vs_transformers(tiny, gold):
    from tests.golden.gen_golden_fallback import windows
    gk = _gk(gold)
    n_last = len(gk["temperature"]) - 1
    pipe = _pipe(tiny, 1)
    try:
        assert any(w["falls_back"] for w in gold["windows"]) and not all(w["falls_back"] for w in gold["windows"])
        for k, (x, w) in enumerate(zip(windows(), gold["windows"])):
            out = pipe(x, generate_kwargs=dict(gk))
            trace = pipe.stats["fallback"]
            mine = [r for r in trace if r["temperature_index"] == 0]
            assert len(mine) >= len(w["passes"])
            for r, want in zip(mine, w["passes"]):
                print(k, r["seek"], r["decision"], r["compression_ratio"], want["compression_ratio"], r["avg_logprob"],
                      want["avg_logprob"], r["no_speech_prob"], want["no_speech_prob"])
                assert r["tokens"].tolist() == want["tokens"]
                assert r["compression_ratio"] == want["compression_ratio"]
                assert abs(r["avg_logprob"] - want["avg_logprob"]) <= 2e-3
                assert abs(r["no_speech_prob"] - want["no_speech_prob"]) <= 1e-4 * max(1.0, want["no_speech_prob"]) + 1e-7
                assert r["decision"] == want["decision"]
            if not w["falls_back"]:
                assert all(r["decision"] != "fallback" for r in trace) and len(mine) == len(w["passes"])
                assert out["text"] == w["text"]
                ok, why = Hh.words_equal(out["chunks"], w["chunks"], tol=0.02)
                assert ok, why
            else:
                # every window the loop saw ends in a kept (or skipped) decode that satisfies the thresholds or is the last one
                by_win = {}
                for r in trace:
                    by_win.setdefault((r["item"], r["seek"]), []).append(r)
                assert any(len(rs) > 1 for rs in by_win.values())
                for rs in by_win.values():
                    assert [r["temperature_index"] for r in rs] == list(range(len(rs)))
                    assert all(r["decision"] == "fallback" for r in rs[:-1])
                    assert rs[-1]["decision"] in ("keep", "skip")
                    assert not rs[-1]["needs_fallback"] or rs[-1]["temperature_index"] == n_last
    finally:
        pipe.engine.close()


def test_kept_result_of_a_fallen_back_window_is_exact_and_carries_its_own_timestamps(tiny, gold):
    """The first pass of every window that falls back at once, through generation._decode_with_fallback on one row under
    cw_set_logits_capture: the capture then holds the logits of the decode that settled the row."""
    from tests.golden.gen_golden_fallback import windows
    g, v, W, spec = tiny
    gk = _gk(gold)
    temps = gk["temperature"]
    pipe = _pipe(tiny, 1)
    eng = pipe.engine
    n_prompt, steps, seed = 3, gk["max_new_tokens"], 4242
    picked = [k for k, w in enumerate(gold["windows"]) if w["passes"][0]["decision"] == "fallback"]
    assert picked
    n_steps = n_close = 0
    try:
        for k in picked:
            x = windows()[k]
            _, nf = eng.mel([x])
            eng.encode([0], [0], [3000])
            eng.set_thresholds(gk["logprob_threshold"], gk["no_speech_threshold"])
            nsp = eng.no_speech_probs(1, v.sot)
            init = np.array([[v.sot, v.lang_id("en"), v.transcribe]], np.int32)
            st = {}
            cap = eng.capture_logits(1, steps)
            try:
                kept = generation._decode_with_fallback(
                    eng, spec, {"temps": temps, "seed": seed, "item_ids": [k], "cr_thr": gk["compression_ratio_threshold"]}, [0],
                    init, n_prompt, n_prompt + steps, 0, np.asarray(nf, np.int64), np.array([0]), nsp, gk["logprob_threshold"],
                    gk["no_speech_threshold"], st)
                cap = cap.copy()
            finally:
                eng.stop_capture()
            last = st["fallback"][-1]
            ti = last["temperature_index"]
            assert ti >= 1 and (not last["needs_fallback"] or ti == len(temps) - 1)
            toks = last["tokens"]                           # padding stripped, eos kept
            stream = generation.stream_id(k, 0, ti)
            ids = init[0].tolist()
            results = []
            for j, t in enumerate(toks.tolist()):
                results.append(R.check_token(spec, cap[j, 0], ids, n_prompt, t, temps[ti], seed, stream))
                ids.append(t)
            wrong = [d for r, d in results if r == "wrong"]
            close = sum(1 for r, _ in results if r == "close")
            print(k, "settled at index", ti, "tokens", len(toks), "left out", close, "ended with eos", toks[-1] == spec.eos_token_id)
            assert not wrong, wrong[:3]
            n_steps += len(results)
            n_close += close
            s, ts_row, skip = kept[0]
            assert not skip and s.tolist() == [t for t in toks.tolist() if t != spec.eos_token_id]
            # the same ids force-aligned (cw_align_tokens, the call behind pipe.align, on the decoder row exactly as the decode
            # left it: the last id is only predicted, whether it is the eos or the token at which max_new_tokens cut the row --
            # pipe.align itself would append an eos to such a row and align one position more): the timestamps of the kept
            # result are those of the decode that produced it, not of the greedy decode before it
            eng.mel([x])
            row = np.asarray(ids, np.int64)
            ali = eng.align_tokens(nf, [row], n_prompt)[0]
            mine = ts_row[:len(row)]
            print("max |ts - aligned|", float(np.abs(mine - ali).max()))
            assert np.abs(mine - ali).max() <= 0.02 + 1e-6
            first = st["fallback"][0]["tokens"].tolist()
            assert first != toks.tolist()
        assert n_close <= 0.01 * n_steps, (n_close, n_steps)
    finally:
        eng.set_thresholds(None, None)
        eng.close()


def test_pipeline_output_does_not_depend_on_batch_size_and_depends_on_the_seed(tiny, gold):
    from tests.golden.gen_golden_thresholds import audio
    gk = _gk(gold)
    x = audio()
    outs, traces = {}, {}
    for name, bs, kw, call in (("b1", 1, {}, {}), ("b8", 8, {}, {}), ("seed", 8, {"sampling_seed": 5}, {}), ("call", 8, {}, {"sampling_seed": 5})):
        pipe = _pipe(tiny, bs, **kw)
        try:
            outs[name] = pipe(x, generate_kwargs=dict(gk), **call)
            traces[name] = pipe.stats["fallback"]
        finally:
            pipe.engine.close()
    assert any(r["decision"] == "fallback" for r in traces["b1"])
    assert outs["b1"] == outs["b8"]
    key = lambda tr: [(r["item"], r["seek"], r["temperature_index"], r["tokens"].tolist(), r["decision"]) for r in tr]
    assert key(traces["b1"]) == key(traces["b8"])
    assert outs["seed"] == outs["call"] and key(traces["seed"]) == key(traces["call"])
    # same decisions and tokens at temperature 0 whatever the seed; a different draw on at least one fallen-back window
    t0 = lambda tr: [e for e in key(tr) if e[2] == 0 and e[1] == 0]
    assert t0(traces["b8"]) == t0(traces["seed"])
    drawn = lambda tr: {(e[0], e[1], e[2]): e[3] for e in key(tr) if e[2] > 0}
    a, b = drawn(traces["b8"]), drawn(traces["seed"])
    assert any(a[k] != b[k] for k in a.keys() & b.keys())
