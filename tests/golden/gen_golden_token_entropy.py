"""Generates tests/golden/token_entropy_golden.json: the predictive entropy of every step of transformers' OWN greedy output
(5.15.0, CPU, fp32) on the tiny synthetic model (gen_golden.build_tiny), for tests/test_gpu_token_entropy.py and
tests/test_gpu_score_entropy.py.

Per clip (each decodes in one pass of the seek loop, as in gen_golden_token_logprobs.py) greedy `generate(output_logits=True,
return_dict_in_generate=True)` gives the generated tokens and the RAW logits of every step -- before suppress lists, the timestamp
rule or any other processor.  One teacher-forced forward over <|startoftranscript|><|en|><|transcribe|> ++ tokens ++ eos gives the
same rows once more (asserted to agree with the free-running ones to 1e-4) and the row that predicts the eos.  Per position, in
float64 on the teacher-forced row x[0 .. V-1], p = softmax(x):

    entropy   H = -sum p log p                       (= log S - Zc / S of include/crisperwhisper.h)
    slope     sum_v p_v |log p_v + H|                dH/dx_v = -p_v (log p_v + H): what an error of delta in every logit moves H by,
    curve     1 + sum_v p_v (log p_v + H)^2          to first order, and the bound on the second-order remainder
                                                     (tests/token_entropy_refs.first_order computes the same from logits)
    bound     the derived error bound of the kernels' f32 evaluation of H on this row (tests/token_entropy_refs.bound), the larger
              of the sampler's and the row kernel's summation depths

    python -m tests.golden.gen_golden_token_entropy
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from crisperwhisper_amd import synthetic as syn
from tests.golden import hf_synth as H
from tests.golden.gen_golden import build_tiny
from tests import token_entropy_refs as R
from tests.golden.gen_golden_token_logprobs import CLIPS

OUT = os.path.dirname(os.path.abspath(__file__))


def stats(row):
    x = np.asarray(row, np.float64)
    lp = x - x.max()
    lp = lp - np.log(np.exp(lp).sum())
    p = np.exp(lp)
    Hh = float(-(p * lp).sum())
    V = len(x)
    bound = max(R.bound(x, V), R.bound(x, V, ((V + 255) // 256, 6 + 4)))
    return Hh, float((p * np.abs(lp + Hh)).sum()), float(1.0 + (p * (lp + Hh) ** 2).sum()), float(bound)


def main():
    g, v, W, model = build_tiny()
    fe = H.build_feature_extractor(g)
    init = [v.sot, v.lang_id("en"), v.transcribe]
    cases = []
    for seed, secs, kind, max_new in CLIPS:
        x = syn.synth_audio(seed, int(round(secs * 16000)), kind)
        feats = fe(x, sampling_rate=16000, return_tensors="pt", return_attention_mask=True).input_features
        with torch.no_grad():
            out = model.generate(input_features=feats, language="<|en|>", task="transcribe", max_new_tokens=max_new, num_beams=1,
                                 return_timestamps=True, return_dict_in_generate=True, output_logits=True)
        seq = [int(t) for t in out["sequences"][0].tolist()]
        if seq[:len(init)] == init:
            seq = seq[len(init):]
        while seq and seq[-1] == v.eos:                              # padding / eos behind the segment
            seq.pop()
        assert seq and all(0 <= t < g.vocab and t != v.eos for t in seq)
        # Whisper's generate hands the underlying call's result to every segment it cut from it: one pass, one result
        res = out["segments"][0][0]["result"]
        assert all(sg["result"] is res for sg in out["segments"][0]), f"clip {seed}: more than one pass of the seek loop"
        free = torch.stack([l.reshape(-1).float() for l in res["logits"]])[:len(seq)]
        with torch.no_grad():
            logits = model(input_features=feats, decoder_input_ids=torch.tensor([init + seq + [v.eos]])).logits[0].float()
        rows = logits[len(init) - 1: len(init) + len(seq)]           # one row per token, and the one that predicts the eos
        assert rows.shape[0] == len(seq) + 1 and rows.shape[1] == g.vocab
        gap = float((rows[:len(seq)] - free).abs().max())
        assert gap < 1e-4, f"clip {seed}: free-running and teacher-forced raw logits differ by {gap}"
        st = [stats(r.numpy()) for r in rows]
        cases.append({"clip": {"seed": seed, "secs": secs, "kind": kind}, "max_new_tokens": max_new, "ids": seq,
                      "entropy": [s[0] for s in st], "slope": [s[1] for s in st], "curve": [s[2] for s in st], "bound": [s[3] for s in st]})
        print(seed, len(seq), "tokens, entropies", [round(s[0], 4) for s in st], "free vs forced", gap)
    json.dump({"init": init, "eos": int(v.eos), "vocab": int(g.vocab), "cases": cases},
              open(os.path.join(OUT, "token_entropy_golden.json"), "w"), ensure_ascii=True, indent=0)


if __name__ == "__main__":
    main()
