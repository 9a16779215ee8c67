"""Generates tests/golden/align_heads_golden.json: per-head forced alignment by transformers (5.15.0, CPU, fp32) on the tiny model
and on the 3-layer x 4-head model of tests/align_heads_models.py, for tests/test_gpu_align_heads_golden.py.

For every model and clip, one teacher-forced eager forward over <|startoftranscript|><|en|><|transcribe|> ++ text gives the
cross-attentions; WhisperGenerationMixin._extract_token_timestamps(..., alignment_heads=[[l, h]], ...) turns them into token
timestamps for every (layer, head) on its own and for the configured heads together, and tokenizer._decode_asr into word chunks.

Conditioning.  A (case, head) pair is ill-conditioned when transformers' own timestamps move by more than 20 ms under a relative
perturbation of 1e-6 of the attention rows (three seeded perturbations; the synthetic non-alignment heads are nearly flat, so
their z-scores amplify rounding).  No engine is asked to reproduce those.  Asserted here: no pair of a designed alignment head
(synthetic.alignment_heads) is ill-conditioned, and at most half of the other pairs are.

Ranking.  The ranking CrisperWhisperPipeline.rank_alignment_heads defines (crisperwhisper_amd.metrics), computed from
transformers' per-head word chunks against the word chunks of the configured heads, with the similarity from the float64
definition (tests/align_heads_refs.py) on transformers' attention rows, clip 200 frames.  `designed_first` records whether the
designed heads lead it.

    python -m tests.golden.gen_golden_align_heads
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from crisperwhisper_amd import metrics, synthetic as syn
from tests import align_heads_models as M
from tests import align_heads_refs as R

OUT = os.path.dirname(os.path.abspath(__file__))
CLIPS = [(41, 30.0, "mixed", 40), (43, 4.0, "chirp", 17), (44, 12.5, "mixed", 24)]      # seed, seconds, kind, ids in the row
TOP = {"tiny": 2, "mid": 3}
COLLAR = 0.05
CLIP_FRAMES = 200


class _Out(dict):
    __getattr__ = dict.__getitem__


def _timestamps(model, dec_in, cross, heads, nf):
    return model._extract_token_timestamps(_Out(sequences=dec_in, cross_attentions=(cross,)), heads, num_frames=[nf],
                                           num_input_ids=3)[0].numpy()


def _chunks(tok, text, ts):
    t_text = torch.from_numpy(np.ascontiguousarray(ts[3:3 + len(text)], np.float32))[None]
    _, extra = tok._decode_asr([{"tokens": torch.tensor([text]), "token_timestamps": t_text}], return_timestamps="word",
                               return_language=None, time_precision=0.02)
    return [{"text": c["text"], "timestamp": [float(c["timestamp"][0]), float(c["timestamp"][1])]} for c in extra["chunks"]]


def _word_groups(tok, text):
    """Token positions of every word, as the tokenizer's word split groups them (a token that starts with a space opens one)."""
    groups, cur = [], []
    for i, t in enumerate(text):
        if cur and tok.decode([t]).startswith(" "):
            groups.append(cur)
            cur = []
        cur.append(i)
    if cur:
        groups.append(cur)
    return groups


def main():
    out = {"collar": COLLAR, "clip_frames": CLIP_FRAMES, "models": {}}
    for name in ("tiny", "mid"):
        g, v, W, spec, model, tok, fe = M.hf_model(name)
        heads = M.all_heads(g)
        designed = [list(h) for h in spec.alignment_heads]
        cases = []
        for seed, secs, kind, n in CLIPS:
            x = syn.synth_audio(seed, int(round(secs * 16000)), kind)
            r = fe(x, sampling_rate=16000, return_tensors="pt", return_attention_mask=True)
            nf = int(r.attention_mask.sum())
            ids = M.rows(v, [n], seed)[0]
            text = [int(t) for t in ids[3:-1]]
            dec_in = torch.tensor([ids[:-1].tolist()])
            with torch.no_grad():
                o = model(input_features=r.input_features, decoder_input_ids=dec_in, output_attentions=True)
            cross = o.cross_attentions
            conf_ts = _timestamps(model, dec_in, cross, designed, nf)
            conf_chunks = _chunks(tok, text, conf_ts)
            groups = _word_groups(tok, text)
            assert len(groups) == len(conf_chunks)
            rb = np.full(len(ids), np.nan, np.float32)
            re = np.full(len(ids), np.nan, np.float32)
            for grp, c in zip(groups, conf_chunks):
                for i in grp:
                    rb[3 + i], re[3 + i] = c["timestamp"]
            n_cols = int(R.ncols_of([nf])[0])
            per_head = []
            for l, h in heads:
                ts = _timestamps(model, dec_in, cross, [[l, h]], nf)
                ill = False
                for ps in range(3):
                    gen = torch.Generator().manual_seed(1000 + ps)
                    pert = tuple(c * (1.0 + 1e-6 * (2.0 * torch.rand(c.shape, generator=gen) - 1.0)) for c in cross)
                    ill = ill or bool(np.abs(_timestamps(model, dec_in, pert, [[l, h]], nf) - ts).max() > 0.02 + 1e-6)
                rows = cross[l][0, h].numpy()
                sim = [R.similarity64(rows[k], n_cols, rb[k], re[k], CLIP_FRAMES) for k in range(3, len(ids) - 1)]
                per_head.append({"head": [l, h], "ill_conditioned": ill, "token_timestamps": [round(float(t), 4) for t in ts],
                                 "chunks": _chunks(tok, text, ts), "similarity": [None if np.isnan(s) else float(s) for s in sim]})
            cases.append({"clip": {"seed": seed, "secs": secs, "kind": kind}, "num_frames": nf, "ids": text,
                          "configured": {"token_timestamps": [round(float(t), 4) for t in conf_ts], "chunks": conf_chunks},
                          "heads": per_head})
        n_des = sum(1 for c in cases for p in c["heads"] if p["head"] in designed)
        ill_des = sum(1 for c in cases for p in c["heads"] if p["head"] in designed and p["ill_conditioned"])
        n_oth = sum(1 for c in cases for p in c["heads"] if p["head"] not in designed)
        ill_oth = sum(1 for c in cases for p in c["heads"] if p["head"] not in designed and p["ill_conditioned"])
        print(f"{name}: ill-conditioned pairs: designed {ill_des} of {n_des}, other {ill_oth} of {n_oth}")
        assert ill_des == 0, "a designed alignment head is ill-conditioned on these clips: pick other clips"
        assert 2 * ill_oth <= n_oth, "more than half of the other pairs are ill-conditioned: pick other clips"
        refs = [np.asarray([c["timestamp"] for c in case["configured"]["chunks"]], np.float64) for case in cases]
        rows = []
        for k in range(len(heads)):
            pred = [np.asarray([c["timestamp"] for c in case["heads"][k]["chunks"]], np.float64) for case in cases]
            sim = [np.asarray([np.nan if s is None else s for s in case["heads"][k]["similarity"]], np.float64) for case in cases]
            rows.append(metrics.head_metrics(pred, refs, sim, collar=COLLAR))
        rk = metrics.rank_heads(heads, rows, top=TOP[name])
        designed_first = sorted(rk["alignment_heads"]) == sorted(designed)      # top = the number of designed heads
        assert len(designed) == TOP[name]
        print(f"{name}: reference ranking {[(r['head'], r['n_within']) for r in rk['ranking']]}; designed first: {designed_first}")
        out["models"][name] = {"designed": designed, "top": TOP[name], "cases": cases, "ranking": rk["ranking"],
                               "alignment_heads": rk["alignment_heads"], "designed_first": bool(designed_first)}
    json.dump(out, open(os.path.join(OUT, "align_heads_golden.json"), "w"), ensure_ascii=True, indent=0)


if __name__ == "__main__":
    main()
