"""Generates tests/golden/token_logprobs_golden.json: per-token log-probabilities of transformers' OWN free-running output
(5.15.0, CPU, fp32) on the tiny synthetic model (gen_golden.build_tiny), for tests/test_gpu_token_logprobs.py.

Per clip (each decodes in one pass of the seek loop -- one generate_with_fallback call: the generator asserts it) and per
search (greedy, 5 beams) the ASR pipeline runs as the e2e golden runs it, and the generate call's `sequences` -- the generated
tokens without the init tokens -- are recorded.
Then ONE teacher-forced forward over <|startoftranscript|><|en|><|transcribe|> ++ sequences gives logits [n_init + n][V];
position p predicts id p + 1, so rows n_init - 1 .. n_init + n - 2 score the n generated tokens:

    logprob    logits.float().log_softmax(-1) gathered at the generated id

which is `logits[tok] - logsumexp(logits[:V])` on the raw logits of the step that produced the token: no suppress lists, no
timestamp rule, no temperature -- what cw_set_token_logprobs stores.

    python -m tests.golden.gen_golden_token_logprobs
"""
from __future__ import annotations

import json
import os

import torch

from crisperwhisper_amd import synthetic as syn
from tests.golden import hf_synth as H
from tests.golden.gen_golden import build_tiny

OUT = os.path.dirname(os.path.abspath(__file__))
# seed, seconds, kind, max_new_tokens.  The random tiny model closes a timestamp pair within ten tokens or so, after which the
# seek loop starts a second pass from the init tokens; six new tokens keep every clip below to ONE pass of the seek loop, for
# both searches (asserted), so one teacher-forced forward over init ++ sequences is the right reference.
CLIPS = [
    (4, 20.0, "mixed", 6),
    (11, 8.0, "noise", 6),
    (3, 5.0, "mixed", 6),
    (13, 6.0, "mixed", 6),
    (5, 15.0, "noise", 6),
    (30, 25.0, "mixed", 6),
]
SEARCHES = {"greedy": 1, "beam5": 5}


def main():
    g, v, W, model = build_tiny()
    tok = H.build_tokenizer(v)
    fe = H.build_feature_extractor(g)
    init = [v.sot, v.lang_id("en"), v.transcribe]
    cases = []
    for seed, secs, kind, max_new in CLIPS:
        x = syn.synth_audio(seed, int(round(secs * 16000)), kind)
        feats = fe(x, sampling_rate=16000, return_tensors="pt", return_attention_mask=True).input_features
        for name, beams in SEARCHES.items():
            pipe = H.build_pipeline(model, tok, fe, batch_size=1)
            calls, passes = [], []
            orig, orig_fb = model.generate, model.generate_with_fallback

            def spy(*a, **k):
                out = orig(*a, **k)
                calls.append(out)
                return out

            def spy_fb(*a, **k):
                passes.append(1)
                return orig_fb(*a, **k)

            model.generate, model.generate_with_fallback = spy, spy_fb
            try:
                res = pipe(x.copy(), generate_kwargs={"num_beams": beams, "language": "<|en|>", "task": "transcribe",
                                                      "max_new_tokens": max_new})
            finally:
                model.generate, model.generate_with_fallback = orig, orig_fb
            assert len(calls) == 1 and len(passes) == 1, f"clip {seed} / {name}: {len(calls)} generate calls, {len(passes)} passes"
            seq = [int(t) for t in calls[0]["sequences"][0].tolist()]
            while seq and seq[-1] == v.eos:                              # padding / eos behind the segment
                seq.pop()
            assert seq and all(0 <= t < g.vocab and t != v.eos for t in seq)
            with torch.no_grad():
                logits = model(input_features=feats, decoder_input_ids=torch.tensor([init + seq])).logits[0].float()
            rows = logits[len(init) - 1: len(init) - 1 + len(seq)]
            lp = rows.log_softmax(-1).gather(1, torch.tensor(seq)[:, None])[:, 0]
            cases.append({"clip": {"seed": seed, "secs": secs, "kind": kind}, "search": name, "num_beams": beams,
                          "max_new_tokens": max_new, "ids": seq, "logprob": [float(a) for a in lp], "text": res["text"]})
            print(seed, name, len(seq), "tokens, sum", float(lp.double().sum()))
    json.dump({"init": init, "eos": int(v.eos), "cases": cases}, open(os.path.join(OUT, "token_logprobs_golden.json"), "w"),
              ensure_ascii=True, indent=0)


if __name__ == "__main__":
    main()
