"""Generates tests/golden/sequence_bias_golden.json: transformers' OWN greedy output (CPU, fp32) under ``sequence_bias`` on the tiny
synthetic model (gen_golden.build_tiny), for tests/test_gpu_sequence_bias.py.

The greedy clips of token_logprobs_golden.json with max_new_tokens = 6 (one pass of the seek loop each) run through the ASR
pipeline once per table of ``tables`` below, with ``generate_kwargs={"sequence_bias": table, "num_beams": 1, ...}``; the generate
call's `sequences` are recorded.  The last logits processor of the list (WhisperTimeStampLogitsProcessor; the list is SequenceBias
-> SuppressTokens -> SuppressTokensAtBegin -> WhisperTimeStamp) is spied on: at every step the gap between the two best
processed scores must exceed GOLD_GAP of tests/top_logprob_refs.py, so that a float32 engine has to pick the same token, and
every case must differ from the clip's unbiased output.  Both are asserted here for every case: none is left out.

    python -m tests.golden.gen_golden_sequence_bias
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from crisperwhisper_amd import synthetic as syn
from tests.golden import hf_synth as H
from tests.golden.gen_golden import build_tiny
from tests.top_logprob_refs import GOLD_GAP

OUT = os.path.dirname(os.path.abspath(__file__))
TEXT = 37                       # '%': a text byte on no suppress list


def tables(v, base):
    """name -> sequence_bias (list form) for a clip whose unbiased output is ``base`` = [ts, text, ...]."""
    tb = v.timestamp_begin
    return {
        "single_token": [[[TEXT], 30.0]],
        "prefix_in_the_baseline": [[[base[1], TEXT], 30.0]],
        "prompt_anchored": [[[v.transcribe, tb + 33], 40.0]],
        "timestamp_token": [[[tb + 400], 35.0]],
        "negative_on_a_baseline_token": [[[base[0]], -30.0]],
        "two_sequences_one_last_token": [[[base[1], TEXT], 22.0], [[base[0], base[1], TEXT], 13.0]],
    }


def main():
    from transformers.generation import logits_process as LP
    g, v, W, model = build_tiny()
    tok = H.build_tokenizer(v)
    fe = H.build_feature_extractor(g)
    src = json.load(open(os.path.join(OUT, "token_logprobs_golden.json")))
    init = src["init"]
    assert init == [v.sot, v.lang_id("en"), v.transcribe]
    cases = []
    for c in src["cases"]:
        if c["search"] != "greedy":
            continue
        assert c["max_new_tokens"] == 6
        x = syn.synth_audio(c["clip"]["seed"], int(round(c["clip"]["secs"] * 16000)), c["clip"]["kind"])
        for name, table in tables(v, c["ids"]).items():
            pipe = H.build_pipeline(model, tok, fe, batch_size=1)
            calls, gaps, kinds = [], [], []
            orig = model.generate
            orig_ts = LP.WhisperTimeStampLogitsProcessor.__call__
            orig_list = LP.LogitsProcessorList.__call__

            def spy(*a, **k):
                out = orig(*a, **k)
                calls.append(out)
                return out

            def spy_ts(self, input_ids, scores):
                out = orig_ts(self, input_ids, scores)
                top = torch.topk(out[0].float(), 2).values
                gaps.append(float(top[0] - top[1]))
                return out

            def spy_list(self, input_ids, scores, **kw):
                kinds.append([type(p).__name__ for p in self])
                return orig_list(self, input_ids, scores, **kw)

            model.generate = spy
            LP.WhisperTimeStampLogitsProcessor.__call__ = spy_ts
            LP.LogitsProcessorList.__call__ = spy_list
            try:
                pipe(x.copy(), generate_kwargs={"num_beams": 1, "language": "<|en|>", "task": "transcribe",
                                                "max_new_tokens": c["max_new_tokens"], "sequence_bias": table})
            finally:
                model.generate = orig
                LP.WhisperTimeStampLogitsProcessor.__call__ = orig_ts
                LP.LogitsProcessorList.__call__ = orig_list
            assert len(calls) == 1, f"clip {c['clip']['seed']} / {name}: {len(calls)} generate calls"
            order = [k for k in kinds if "SequenceBiasLogitsProcessor" in k]
            assert order and all(k[0] == "SequenceBiasLogitsProcessor" and k[-1] == "WhisperTimeStampLogitsProcessor" for k in order), kinds[:2]
            seq = [int(t) for t in calls[0]["sequences"][0].tolist()]
            while seq and seq[-1] == v.eos:
                seq.pop()
            assert seq and seq != c["ids"], f"clip {c['clip']['seed']} / {name}: the table changes nothing"
            assert len(gaps) >= len(seq) and min(gaps) > GOLD_GAP, f"clip {c['clip']['seed']} / {name}: gap {min(gaps)}"
            cases.append({"clip": c["clip"], "name": name, "max_new_tokens": c["max_new_tokens"], "sequence_bias": table,
                          "baseline": c["ids"], "ids": seq, "min_gap": min(gaps)})
            print(c["clip"]["seed"], name, c["ids"], "->", seq, "min gap", round(min(gaps), 4))
    json.dump({"init": init, "eos": int(v.eos), "gap": GOLD_GAP, "cases": cases},
              open(os.path.join(OUT, "sequence_bias_golden.json"), "w"), ensure_ascii=True, indent=0)


if __name__ == "__main__":
    main()
