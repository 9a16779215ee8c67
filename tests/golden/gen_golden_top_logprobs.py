"""Generates tests/golden/top_logprobs_golden.json: the six most probable tokens of every step of transformers' OWN greedy
output (CPU, fp32) on the tiny synthetic model (gen_golden.build_tiny), for tests/test_gpu_top_logprobs.py.

The greedy cases of token_logprobs_golden.json (gen_golden_token_logprobs.py: one seek-loop pass each) are taken as they are.
Per case ONE teacher-forced forward over <|startoftranscript|><|en|><|transcribe|> ++ ids gives logits [n_init + n][V]; rows
n_init - 1 .. n_init + n - 2 are the raw logits of the steps that produced the n generated tokens, and per row

    top_ids, top_logprobs    logits.float().log_softmax(-1).topk(6), ties to the lower id

-- no suppress lists, no timestamp rule, no temperature: what cw_set_top_logprobs stores.  Six are recorded for a test of five:
rank j of a float32 engine is held to the golden only where the golden's gaps to both neighbours (ranks j - 1 and j + 1) exceed
GAP = twice the float32 bound of tests/test_gpu_score_vs_transformers.py, since a smaller gap may legitimately swap two ids.
The generator asserts what the test asserts: at most 10 % of the (position, rank) pairs fail that gap test.

    python -m tests.golden.gen_golden_top_logprobs
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from crisperwhisper_amd import synthetic as syn
from tests.golden import hf_synth as H
from tests.golden.gen_golden import build_tiny
from tests.top_logprob_refs import GOLD_GAP as GAP, GOLD_K as K_TEST, GOLD_MAX_LEFT_OUT as MAX_LEFT_OUT, checked_pairs

OUT = os.path.dirname(os.path.abspath(__file__))
N_TOP = 6


def main():
    g, v, W, model = build_tiny()
    fe = H.build_feature_extractor(g)
    src = json.load(open(os.path.join(OUT, "token_logprobs_golden.json")))
    init = src["init"]
    assert init == [v.sot, v.lang_id("en"), v.transcribe]
    cases, n_pairs, n_checked, n_rank0, n_rank0_checked = [], 0, 0, 0, 0
    for c in src["cases"]:
        if c["search"] != "greedy":
            continue
        x = syn.synth_audio(c["clip"]["seed"], int(round(c["clip"]["secs"] * 16000)), c["clip"]["kind"])
        feats = fe(x, sampling_rate=16000, return_tensors="pt", return_attention_mask=True).input_features
        seq = c["ids"]
        with torch.no_grad():
            logits = model(input_features=feats, decoder_input_ids=torch.tensor([init + seq])).logits[0].float()
        lsm = logits[len(init) - 1: len(init) - 1 + len(seq)].log_softmax(-1).numpy()
        ids = np.stack([np.lexsort((np.arange(lsm.shape[1]), -row))[:N_TOP] for row in lsm])
        lps = np.take_along_axis(lsm, ids, axis=1)
        own = np.array([lsm[p, t] for p, t in enumerate(seq)])
        assert np.allclose(own, np.asarray(c["logprob"]), rtol=0, atol=1e-5), "not the forward the token golden came from"
        ok = checked_pairs(lps)
        n_pairs += ok.size; n_checked += int(ok.sum()); n_rank0 += len(ok); n_rank0_checked += int(ok[:, 0].sum())
        cases.append({"clip": c["clip"], "max_new_tokens": c["max_new_tokens"], "ids": seq,
                      "top_ids": ids.tolist(), "top_logprobs": [[float(a) for a in r] for r in lps]})
        print(c["clip"]["seed"], len(seq), "positions,", int((~ok).sum()), "pairs left out")
    print(f"left out: {n_pairs - n_checked} of {n_pairs} pairs at k = {K_TEST}, {n_rank0 - n_rank0_checked} of {n_rank0} at rank 0")
    assert n_pairs - n_checked <= MAX_LEFT_OUT * n_pairs
    json.dump({"init": init, "eos": int(v.eos), "n_top": N_TOP, "k": K_TEST, "gap": GAP, "max_left_out": MAX_LEFT_OUT,
               "cases": cases}, open(os.path.join(OUT, "top_logprobs_golden.json"), "w"), ensure_ascii=True, indent=0)


if __name__ == "__main__":
    main()
