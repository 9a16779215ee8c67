"""CrisperWhisperPipeline.score(top_logprobs=8) against transformers on the tiny geometry (tests/golden/gen_golden_score_top.py):
for the transcripts of the score golden that pass the generator's own condition, the reference's 16 most probable tokens of every
teacher-forced position, by `logits.float().log_softmax(-1)` on the CPU in fp32.

Gates, with the per-token bounds of tests/test_gpu_score_vs_transformers.py (4e-3 f32, 0.08 f16, 0.5 bf16: twice the logit bound,
which holds for any token's log-probability, not the target's only).
f32 engine: rank j < 8 of a position is comparable when the reference's gaps to ranks j - 1 and j + 1 both exceed twice the f32
bound; no engine within the bound can order such a rank differently, so comparable ranks must carry the reference's id (and its
log-probability within the bound).  At most 10 % of the (position, rank) pairs are not comparable -- a condition on the golden
that the generator asserts when it writes the file and that is asserted again here.
16-bit engines: every returned id that the reference lists within its 16 has its log-probability within the engine's bound; an
id the reference does not list is below the reference's 16th, so it must not exceed that by more than the bound.
"""
import numpy as np
import pytest

import crisperwhisper_amd as cw
from crisperwhisper_amd import collate, synthetic as syn
from tests import helpers as Hh
from tests.test_gpu_score_vs_transformers import BOUND

pytestmark = pytest.mark.gpu

GOLD = Hh.gold_json("e2e_score_top_golden.json")
K = 8


def _comparable(lp):
    gap = lp[:, :-1] - lp[:, 1:]
    ok = gap[:, :K] > GOLD["gap"]
    ok[:, 1:] &= gap[:, :K - 1] > GOLD["gap"]
    return ok


def test_golden_satisfies_its_own_condition():
    assert GOLD["k"] == K and GOLD["n_ref"] == 16 and GOLD["gap"] == 2 * BOUND["float32"]
    n = bad = 0
    for c in GOLD["cases"]:
        ok = _comparable(np.asarray(c["top_logprobs"], np.float64))
        n += ok.size; bad += int((~ok).sum())
    assert (n, bad) == (GOLD["n_pairs"], GOLD["n_incomparable"]) and bad <= 0.10 * n


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
def test_score_top_vs_transformers(dtype):
    g, v, W, spec = Hh.tiny_setup()
    assert GOLD["init"] == [v.sot, v.lang_id("en"), v.transcribe] and GOLD["eos"] == v.eos
    by_clip = {}
    for c in GOLD["cases"]:
        by_clip.setdefault(c["clip"]["seed"], []).append(c)
    clips_cases = list(by_clip.values())
    clips = [syn.synth_audio(cs[0]["clip"]["seed"], int(round(cs[0]["clip"]["secs"] * 16000)), cs[0]["clip"]["kind"])
             for cs in clips_cases]
    cands = [[c["ids"] for c in cs] for cs in clips_cases]
    pipe = cw.pipeline("automatic-speech-recognition", model=cw.ModelBundle(spec, W), tokenizer=collate.Vocabulary.from_synthetic(v),
                       batch_size=4, return_timestamps="word", torch_dtype=dtype, device="cuda:0")
    bound = BOUND[dtype]
    try:
        got = pipe.score(clips, cands, language="<|en|>", task="transcribe", top_logprobs=K)
        worst = 0.0
        listed = unlisted = matched = n_cmp = 0
        for cases, res in zip(clips_cases, got):
            for c, r in zip(cases, res):
                ref_id = np.asarray(c["top_ids"]); ref_lp = np.asarray(c["top_logprobs"], np.float64)
                assert [t["id"] for t in r["tokens"]] == c["ids"] + [GOLD["eos"]] and len(r["tokens"]) == len(ref_id)
                ok = _comparable(ref_lp)
                for p, t in enumerate(r["tokens"]):
                    top = t["top_logprobs"]
                    assert len(top) == K
                    for j, e in enumerate(top):
                        w = np.flatnonzero(ref_id[p] == e["id"])
                        if w.size:
                            d = abs(e["logprob"] - ref_lp[p, w[0]])
                            worst = max(worst, d)
                            listed += 1
                            assert d <= bound, (dtype, c["name"], p, j, e, float(ref_lp[p, w[0]]))
                        else:
                            unlisted += 1
                            assert e["logprob"] <= ref_lp[p, -1] + bound, (dtype, c["name"], p, j, e, float(ref_lp[p, -1]))
                        if dtype == "float32" and ok[p, j]:
                            n_cmp += 1
                            assert e["id"] == ref_id[p, j], (c["name"], p, j, e, int(ref_id[p, j]))
                        matched += int(e["id"] == ref_id[p, j])
        print(dtype, "worst |logprob - ref| over", listed, "listed alternatives:", worst, "; not in the reference's 16:", unlisted,
              "; rank for rank equal:", matched, "of", listed + unlisted, "; comparable ranks checked:", n_cmp)
        if dtype == "float32":
            assert n_cmp == GOLD["n_pairs"] - GOLD["n_incomparable"]
    finally:
        pipe.engine.close()
