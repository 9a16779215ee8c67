"""Generates tests/golden/e2e_align_golden.json: forced alignment of known transcripts by transformers (5.15.0, CPU, fp32) on the
tiny synthetic model (the one gen_golden.build_tiny makes), for tests/test_gpu_align_vs_transformers.py.

For every case the decoder input is <|startoftranscript|><|en|><|transcribe|> ++ transcript.  One teacher-forced forward of the
model over exactly that input (eager attention, output_attentions=True) gives the cross-attentions, and
WhisperGenerationMixin._extract_token_timestamps turns them into one timestamp per id of init + transcript + eos
(num_input_ids = 3, num_frames from the feature extractor's attention mask).  The words come from tokenizer._decode_asr over the
transcript's ids and their timestamps, with return_timestamps="word".

Transcripts: the model's own text (8 words: a space, then 3 greedy letters, argmax over a-z), the same with every third word
dropped, with neighbouring words swapped, and unrelated text.  Clips: 30 s, 12.5 s, 4 s and 20 s (num_frames 3000, 1250, 400, 2000).

    python -m tests.golden.gen_golden_align
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
CLIPS = [(41, 30.0, "mixed"), (42, 12.5, "noise"), (43, 4.0, "chirp"), (44, 20.0, "mixed")]
UNRELATED = [" the patient was given two tablets of paracetamol", " subtitles for the second act, scene four",
             " uh we measured it again on monday", " ok"]


class _Out(dict):
    __getattr__ = dict.__getitem__


def _words(tok, ids):
    """Word boundaries of a token list: a token whose text starts with a space opens a word."""
    words, cur = [], []
    for t in ids:
        if cur and tok.decode([t]).startswith(" "):
            words.append(cur)
            cur = []
        cur.append(t)
    if cur:
        words.append(cur)
    return words


def main():
    g, v, W, model = build_tiny()
    model.config._attn_implementation = "eager"
    tok = H.build_tokenizer(v)
    fe = H.build_feature_extractor(g)
    init = [v.sot, v.lang_id("en"), v.transcribe]
    heads = model.generation_config.alignment_heads
    letters = torch.arange(ord("a"), ord("z") + 1)                # the tiny vocabulary is bytes
    cases = []
    for ci, (seed, secs, kind) in enumerate(CLIPS):
        x = syn.synth_audio(seed, int(round(secs * 16000)), kind)
        r = fe(x, sampling_rate=16000, return_tensors="pt", return_attention_mask=True)
        feats, nf = r.input_features, int(r.attention_mask.sum())
        with torch.no_grad():
            ids = list(init)
            for k in range(32):                                   # the model's own text: 8 words of greedy letters
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
        for name, text in (("own", own), ("dropped", dropped), ("swapped", swapped), ("unrelated", unrelated)):
            dec_in = torch.tensor([init + text])
            with torch.no_grad():
                o = model(input_features=feats, decoder_input_ids=dec_in, output_attentions=True)
            ts = model._extract_token_timestamps(_Out(sequences=dec_in, cross_attentions=(o.cross_attentions,)), heads,
                                                 num_frames=[nf], num_input_ids=len(init))[0].numpy()
            assert len(ts) == len(init) + len(text) + 1
            t_text = torch.from_numpy(np.ascontiguousarray(ts[3:3 + len(text)], np.float32))[None]
            txt, extra = tok._decode_asr([{"tokens": torch.tensor([text]), "token_timestamps": t_text}],
                                         return_timestamps="word", return_language=None, time_precision=0.02)
            cases.append({"clip": {"seed": seed, "secs": secs, "kind": kind}, "name": name, "num_frames": nf,
                          "ids": [int(t) for t in text], "token_timestamps": [round(float(t), 4) for t in ts],
                          "text": txt, "chunks": [{"text": c["text"], "timestamp": [float(c["timestamp"][0]), float(c["timestamp"][1])]}
                                                  for c in extra["chunks"]]})
    json.dump({"init": init, "cases": cases}, open(os.path.join(OUT, "e2e_align_golden.json"), "w"), ensure_ascii=True, indent=0)


if __name__ == "__main__":
    main()
