"""Generates tests/golden/e2e_score_top_golden.json: the 16 most probable tokens of every teacher-forced position by transformers
(5.15.0, CPU, fp32) on the tiny synthetic model, for tests/test_gpu_score_top_vs_transformers.py.

Clips and transcripts are those of e2e_score_golden.json (gen_golden_score).  For every case the decoder input is
<|startoftranscript|><|en|><|transcribe|> ++ transcript; position p predicts id p + 1 of init ++ transcript ++ eos.  Recorded per
case, for the n text tokens and the eos: "top_ids" / "top_logprobs" [n + 1][16] -- logits.float().log_softmax(-1), sorted by
value descending, id ascending on an exact tie.

Rank j < 8 of a position is comparable when the reference's gaps to ranks j - 1 and j + 1 both exceed GAP = twice the f32
per-token bound of tests/test_gpu_score_vs_transformers.py (an engine within that bound cannot order such a rank differently).
The generator asserts what the test needs of the reference alone: at most 10 % of all (position, rank < 8) pairs are not
comparable.  Cases are taken in the order of the score golden and a case is left out when it alone has more than 10 % -- the
kept ones are listed by clip seed and name.

    python -m tests.golden.gen_golden_score_top
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from crisperwhisper_amd import synthetic as syn
from tests.golden import hf_synth as H
from tests.golden.gen_golden import build_tiny

OUT = os.path.dirname(os.path.abspath(__file__))
N_REF = 16
K = 8
GAP = 8e-3               # twice the f32 per-token log-probability bound (4e-3)


def comparable(lp):
    """lp [n][N_REF] descending -> bool [n][K]: both neighbouring gaps of rank j exceed GAP (rank 0 has one neighbour)."""
    gap = lp[:, :-1] - lp[:, 1:]                                         # gap[j] between ranks j and j + 1
    ok = gap[:, :K] > GAP
    ok[:, 1:] &= gap[:, :K - 1] > GAP
    return ok


def main():
    score = json.load(open(os.path.join(OUT, "e2e_score_golden.json")))
    g, v, W, model = build_tiny()
    fe = H.build_feature_extractor(g)
    init = score["init"]
    cases, n_pairs, n_bad = [], 0, 0
    feats_of = {}
    for c in score["cases"]:
        clip = c["clip"]
        if clip["seed"] not in feats_of:
            x = syn.synth_audio(clip["seed"], int(round(clip["secs"] * 16000)), clip["kind"])
            feats_of[clip["seed"]] = fe(x, sampling_rate=16000, return_tensors="pt", return_attention_mask=True).input_features
        with torch.no_grad():
            logits = model(input_features=feats_of[clip["seed"]], decoder_input_ids=torch.tensor([init + c["ids"]])).logits[0].float()
        lsm = logits[len(init) - 1:].log_softmax(-1).numpy()
        assert lsm.shape[0] == len(c["ids"]) + 1
        ids = np.stack([np.lexsort((np.arange(lsm.shape[1]), -row))[:N_REF] for row in lsm])
        lp = np.take_along_axis(lsm, ids, axis=1)
        assert np.array_equal(ids[:, 0], np.asarray(c["top_id"])) or np.any(np.asarray(c["margin"]) == 0)
        ok = comparable(lp.astype(np.float64))
        bad = int((~ok).sum())
        print(clip["seed"], c["name"], f"{bad} of {ok.size} (position, rank) pairs not comparable")
        if bad > 0.10 * ok.size:
            continue
        n_pairs += ok.size
        n_bad += bad
        cases.append({"clip": clip, "name": c["name"], "ids": c["ids"], "top_ids": ids.astype(int).tolist(),
                      "top_logprobs": [[float(a) for a in row] for row in lp]})
    assert len(cases) >= 4 and len({c["clip"]["seed"] for c in cases}) >= 2, "too few cases pass the reference's own condition"
    assert n_bad <= 0.10 * n_pairs, f"{n_bad} of {n_pairs} (position, rank) pairs are not comparable"
    json.dump({"init": init, "eos": int(v.eos), "gap": GAP, "n_ref": N_REF, "k": K, "n_pairs": n_pairs, "n_incomparable": n_bad,
               "cases": cases}, open(os.path.join(OUT, "e2e_score_top_golden.json"), "w"), ensure_ascii=True, indent=0)
    print(f"{len(cases)} cases, {n_pairs} (position, rank) pairs, {n_bad} not comparable")


if __name__ == "__main__":
    main()
