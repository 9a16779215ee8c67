"""CrisperWhisperPipeline.score against transformers on the tiny geometry (tests/golden/gen_golden_score.py): the 16 transcripts
over 4 clips of the align golden -- the model's own text, the same with words dropped, with words swapped, and unrelated text --
scored by `model(input_features, decoder_input_ids).logits.float().log_softmax(-1)` on the CPU in fp32.  Every clip goes through
one score call with its four candidates (rows_per_item 4), on each engine and on both forward paths where the engine has both.

Gates.  A log-probability is a logit minus a log-sum-exp of logits, so its error is at most twice the logit error; the
teacher-forced logit bounds of test_teacher_forced_decoder on this model (2e-3 f32, 0.04 f16, 0.25 bf16) give 4e-3 / 0.08 / 0.5
per token.  top_id: f32 -- equal to the reference wherever the reference's top-two margin exceeds 4e-3 (the generator caps the
excluded share at 5 %); 16-bit -- agreement on at least 90 % of all positions.  Ranking: per clip the order of its candidates by
logprob and by avg_logprob equals the reference's for every pair the reference separates by more than the per-token bound times
the longer token count (an exact tie in the reference must come out as an exact tie).  Words: chunk texts and token groups
equal the golden's, every chunk logprob the sum of its tokens', logprob / avg_logprob by their formulas.
"""
import numpy as np
import pytest

import crisperwhisper_amd as cw
from crisperwhisper_amd import collate, synthetic as syn
from tests import helpers as Hh

pytestmark = pytest.mark.gpu

GOLD = Hh.gold_json("e2e_score_golden.json")
BOUND = {"float32": 4e-3, "float16": 0.08, "bfloat16": 0.5}


def _check(dtype, path, clips_cases, got):
    bound = BOUND[dtype]
    worst = 0.0
    agree = n_pos = 0
    for cases, res in zip(clips_cases, got):
        assert isinstance(res, list) and len(res) == len(cases)
        for c, r in zip(cases, res):
            ref = np.asarray(c["logprob"]); lp = np.asarray([t["logprob"] for t in r["tokens"]])
            assert [t["id"] for t in r["tokens"]] == c["ids"] + [GOLD["eos"]]
            d = np.abs(lp - ref)
            worst = max(worst, float(d.max()))
            print(dtype, path, c["clip"]["seed"], c["name"], "max |logprob - ref| =", float(d.max()))
            assert np.all(d <= bound), (dtype, path, c["name"], float(d.max()))
            top = np.asarray([t["top_id"] for t in r["tokens"]]); ref_top = np.asarray(c["top_id"])
            if dtype == "float32":
                clear = np.asarray(c["margin"]) > GOLD["margin_bound"]
                assert np.array_equal(top[clear], ref_top[clear]), (path, c["name"])
                dt = np.abs(np.asarray([t["top_logprob"] for t in r["tokens"]]) - np.asarray(c["top_logprob"]))
                assert np.all(dt <= bound)
            agree += int((top == ref_top).sum()); n_pos += len(top)
            # words
            assert [w["text"] for w in r["chunks"]] == c["chunks"], c["name"]
            for w, grp in zip(r["chunks"], c["word_groups"]):
                assert w["logprob"] == pytest.approx(float(lp[grp].sum()), abs=1e-9 + 1e-12 * len(grp))
            assert r["logprob"] == pytest.approx(float(lp.sum()), abs=1e-9)
            assert r["avg_logprob"] == pytest.approx(float(lp.sum()) / (len(c["ids"]) + 1), abs=1e-9)
        # ranking
        pairs = 0
        for a in range(len(cases)):
            for b in range(a + 1, len(cases)):
                ca, cb = cases[a], cases[b]
                na, nb = len(ca["logprob"]), len(cb["logprob"])
                for key, ra, rb, gap in (("logprob", ca["sum_logprob"], cb["sum_logprob"], bound * max(na, nb)),
                                         ("avg_logprob", ca["sum_logprob"] / na, cb["sum_logprob"] / nb, 2 * bound)):
                    if ca["ids"] == cb["ids"]:
                        assert res[a][key] == res[b][key], (path, ca["name"], cb["name"])      # an exact tie stays one
                    elif abs(ra - rb) > gap:
                        pairs += key == "logprob"
                        assert (res[a][key] > res[b][key]) == (ra > rb), (path, key, ca["name"], cb["name"])
        if dtype == "float32":
            assert pairs >= 1
    print(dtype, path, "worst", worst, "top_id agreement", agree / n_pos)
    assert agree >= 0.9 * n_pos


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
def test_score_vs_transformers(dtype):
    g, v, W, spec = Hh.tiny_setup()
    assert GOLD["init"] == [v.sot, v.lang_id("en"), v.transcribe] and GOLD["eos"] == v.eos
    assert GOLD["n_close"] <= 0.05 * GOLD["n_positions"]
    by_clip = {}
    for c in GOLD["cases"]:
        by_clip.setdefault(c["clip"]["seed"], []).append(c)
    clips_cases = list(by_clip.values())
    clips = [syn.synth_audio(cs[0]["clip"]["seed"], int(round(cs[0]["clip"]["secs"] * 16000)), cs[0]["clip"]["kind"])
             for cs in clips_cases]
    cands = [[c["ids"] for c in cs] for cs in clips_cases]
    pipe = cw.pipeline("automatic-speech-recognition", model=cw.ModelBundle(spec, W), tokenizer=collate.Vocabulary.from_synthetic(v),
                       batch_size=4, return_timestamps="word", torch_dtype=dtype, device="cuda:0")
    eng = pipe.engine
    try:
        assert eng.max_batch >= 16
        got = pipe.score(clips, cands, language="<|en|>", task="transcribe")
        if dtype == "float32":
            assert eng.score_prefill_runs() == 0
            _check(dtype, "loop", clips_cases, got)
        else:
            assert eng.score_prefill_runs() == 1                      # 4 items x 4 candidates: one call
            _check(dtype, "prefill", clips_cases, got)
            eng.set_score_prefill(False)
            got_l = pipe.score(clips, cands, language="<|en|>", task="transcribe")
            assert eng.score_prefill_runs() == 1
            _check(dtype, "loop", clips_cases, got_l)
    finally:
        eng.close()
