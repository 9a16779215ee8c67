"""Generates tests/golden/e2e_score_golden.json: teacher-forced token log-probabilities of known transcripts by transformers
(5.15.0, CPU, fp32) on the tiny synthetic model (the one gen_golden.build_tiny makes), for
tests/test_gpu_score_vs_transformers.py and tests/test_score_host.py.

Clips and transcripts are gen_golden_align's: four clips, and per clip the model's own text, the same with every third word
dropped, with neighbouring words swapped, and unrelated text.  For every case the decoder input is
<|startoftranscript|><|en|><|transcribe|> ++ transcript; one forward gives logits [n_init + n][V], and position p predicts id
p + 1 of init ++ transcript ++ eos.  Recorded per case, for the n text tokens and the eos:

    logprob       logits.float().log_softmax(-1) gathered at the next id
    top_id        the arg-max id,  top_logprob  its log-probability
    margin        the gap between the two largest logits of the position
    word_groups   the token index groups of the words (tokenization_whisper._combine_tokens_into_words), and "chunks" their texts

The generator asserts what the tests need of the reference alone: at most 5 % of all scored positions have a top-two margin
below MARGIN (the f32 logit bound doubled), and every clip has at least one pair of candidates whose total log-probabilities
lie further apart than the f32 per-token bound times the longer token count.

    python -m tests.golden.gen_golden_score
"""
from __future__ import annotations

import json
import os

import torch

from crisperwhisper_amd import synthetic as syn
from tests.golden import hf_synth as H
from tests.golden.gen_golden import build_tiny
from tests.golden.gen_golden_align import CLIPS, UNRELATED, _words

OUT = os.path.dirname(os.path.abspath(__file__))
MARGIN = 4e-3            # twice the f32 teacher-forced logit bound (2e-3)
TOKEN_BOUND_F32 = 4e-3   # per-token log-probability bound of the f32 engine


def main():
    from transformers.models.whisper.tokenization_whisper import _combine_tokens_into_words
    g, v, W, model = build_tiny()
    tok = H.build_tokenizer(v)
    fe = H.build_feature_extractor(g)
    init = [v.sot, v.lang_id("en"), v.transcribe]
    letters = torch.arange(ord("a"), ord("z") + 1)
    cases = []
    n_pos = n_close = 0
    for ci, (seed, secs, kind) in enumerate(CLIPS):
        x = syn.synth_audio(seed, int(round(secs * 16000)), kind)
        r = fe(x, sampling_rate=16000, return_tensors="pt", return_attention_mask=True)
        feats, nf = r.input_features, int(r.attention_mask.sum())
        with torch.no_grad():
            ids = list(init)
            for k in range(32):
                if k % 4 == 0:
                    ids.append(ord(" "))
                    continue
                lg = model(input_features=feats, decoder_input_ids=torch.tensor([ids])).logits[0, -1]
                ids.append(int(letters[lg[letters].argmax()]))
        own = ids[3:]
        ws = _words(tok, own)
        dropped = [t for k, w in enumerate(ws) if k % 3 != 1 for t in w]
        swapped = [t for k in range(0, len(ws), 2) for w in (ws[k + 1:k + 2] + ws[k:k + 1]) for t in w]
        unrelated = tok.encode(UNRELATED[ci], add_special_tokens=False)
        clip_cases = []
        for name, text in (("own", own), ("dropped", dropped), ("swapped", swapped), ("unrelated", unrelated)):
            with torch.no_grad():
                logits = model(input_features=feats, decoder_input_ids=torch.tensor([init + text])).logits[0].float()
            rows = logits[len(init) - 1:]                                    # positions that predict text tokens and the eos
            targets = torch.tensor(list(text) + [v.eos])
            assert rows.shape[0] == len(targets)
            lsm = rows.log_softmax(-1)
            lp = lsm.gather(1, targets[:, None])[:, 0]
            top_lp, top_id = lsm.max(-1)
            top2 = rows.topk(2, dim=-1).values
            margin = top2[:, 0] - top2[:, 1]
            n_pos += len(targets)
            n_close += int((margin <= MARGIN).sum())
            words, _, groups = _combine_tokens_into_words(tok, list(text), None)
            clip_cases.append({
                "clip": {"seed": seed, "secs": secs, "kind": kind}, "name": name, "num_frames": nf, "ids": [int(t) for t in text],
                "logprob": [float(a) for a in lp], "top_id": [int(a) for a in top_id], "top_logprob": [float(a) for a in top_lp],
                "margin": [float(a) for a in margin], "chunks": list(words), "word_groups": [[int(i) for i in gidx] for gidx in groups],
                "sum_logprob": float(lp.double().sum())})
        ok = False
        for a in range(len(clip_cases)):
            for b in range(a + 1, len(clip_cases)):
                n = max(len(clip_cases[a]["logprob"]), len(clip_cases[b]["logprob"]))
                ok |= abs(clip_cases[a]["sum_logprob"] - clip_cases[b]["sum_logprob"]) > TOKEN_BOUND_F32 * n
        assert ok, f"clip {seed}: no pair of candidates is separated beyond the f32 bound"
        cases.extend(clip_cases)
    assert n_close <= 0.05 * n_pos, f"{n_close} of {n_pos} positions have a top-two margin <= {MARGIN}"
    json.dump({"init": init, "eos": int(v.eos), "margin_bound": MARGIN, "n_positions": n_pos, "n_close": n_close, "cases": cases},
              open(os.path.join(OUT, "e2e_score_golden.json"), "w"), ensure_ascii=True, indent=0)
    print(f"{len(cases)} cases, {n_pos} positions, {n_close} with margin <= {MARGIN}")


if __name__ == "__main__":
    main()
