"""Golden for temperature fallback (TF generation_whisper.py:970-1116, _need_fallback :1243-1287): the reference pipeline call
with the full temperature tuple, `compression_ratio_threshold`, `logprob_threshold` and `no_speech_threshold`, on the six 30 s
windows (25 s apart) of the recording of gen_golden_thresholds.py, each window transcribed on its own.

Only what transformers computes deterministically is recorded: every temperature-0 decode of a window (one per pass of the seek
loop) with its tokens, compression ratio, average log-probability, no-speech probability and decision.  What follows a
fallback is drawn from torch's generator and is not comparable; a window none of whose passes falls back is deterministic to
the end, and its words are recorded too.

A first run with thresholds that can never fire records the quantities; the compression-ratio threshold is then put into the
widest gap between the windows' largest ratios, so that some windows fall back and others do not; the log-probability and
no-speech thresholds are set where they never fire (their quantities are still computed and compared).

    python -m tests.golden.gen_golden_fallback          (tiny geometry, a few CPU minutes)
Writes tests/golden/e2e_fallback_golden.json."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests.golden import hf_synth as H
from tests.golden.gen_golden import build_tiny
from tests.golden.gen_golden_thresholds import audio

OUT = os.path.dirname(os.path.abspath(__file__))
TEMPERATURES = (0.0, 0.2, 0.4, 0.6, 0.8, 1.0)
N_WINDOWS, WINDOW_STEP, WINDOW = 6, 400000, 480000


def windows():
    x = audio()
    return [x[k * WINDOW_STEP: k * WINDOW_STEP + WINDOW].copy() for k in range(N_WINDOWS)]


def run(model, tok, fe, x, gk, record):
    """One pipeline call on one window; record receives one dict per _need_fallback call."""
    import transformers.models.whisper.generation_whisper as GW
    from transformers.generation.logits_process import WhisperNoSpeechDetection
    pipe = H.build_pipeline(model, tok, fe, batch_size=1)
    orig = model._need_fallback

    def spy(seek_sequence, seek_outputs, index, logits_processor, generation_config, vocab_size, temperature):
        nf, sk = orig(seek_sequence, seek_outputs, index, logits_processor, generation_config, vocab_size, temperature)
        lp = float(model._retrieve_avg_logprobs(seek_outputs[index]["scores"], seek_sequence, temperature))
        nsp = float(GW._get_attr_from_logit_processors(logits_processor, WhisperNoSpeechDetection, "no_speech_prob")[index])
        record.append({"temperature": float(temperature), "tokens": [int(t) for t in seek_sequence.tolist()],
                       "compression_ratio": float(model._retrieve_compression_ratio(seek_sequence, vocab_size)),
                       "avg_logprob": lp, "no_speech_prob": nsp, "needs_fallback": bool(nf), "should_skip": bool(sk)})
        return nf, sk

    model._need_fallback = spy
    try:
        torch.manual_seed(0)
        res = pipe(x.copy(), generate_kwargs=dict(gk))
    finally:
        model._need_fallback = orig
    return {"text": res["text"], "chunks": [{"text": c["text"], "timestamp": list(c["timestamp"])} for c in res["chunks"]]}


def main():
    g, v, W, model = build_tiny()
    tok = H.build_tokenizer(v)
    fe = H.build_feature_extractor(g)
    base = {"num_beams": 1, "language": "<|en|>", "task": "transcribe", "max_new_tokens": 24}
    never = {"compression_ratio_threshold": 1.0e9, "logprob_threshold": -1.0e9, "no_speech_threshold": 2.0}
    probe = []
    for x in windows():
        rec = []
        run(model, tok, fe, x, {**base, "temperature": (0.0,), **never}, rec)
        probe.append(rec)
    top = sorted(max(r["compression_ratio"] for r in rec) for rec in probe)
    gaps = [(b - a, 0.5 * (a + b)) for a, b in zip(top[:-1], top[1:])]
    gap, cr_thr = max(gaps)
    assert gap > 0.02, top
    lp_thr = min(r["avg_logprob"] for rec in probe for r in rec) - 1.0
    gk = {**base, "temperature": TEMPERATURES, "compression_ratio_threshold": cr_thr, "logprob_threshold": lp_thr,
          "no_speech_threshold": 2.0}
    out = {"audio": "tests/golden/gen_golden_fallback.py:windows()", "generate_kwargs": {**gk, "temperature": list(TEMPERATURES)},
           "windows": []}
    for k, x in enumerate(windows()):
        rec = []
        res = run(model, tok, fe, x, gk, rec)
        fell = any(r["needs_fallback"] for r in rec if r["temperature"] == 0.0)
        passes = []
        for r in rec:                                # the temperature-0 decodes up to and including the first that falls back
            if r["temperature"] != 0.0:
                break
            passes.append({**r, "decision": "skip" if r["should_skip"] else ("fallback" if r["needs_fallback"] else "keep")})
            if r["needs_fallback"]:
                break
        w = {"falls_back": bool(fell), "passes": passes}
        if not fell:
            assert all(r["temperature"] == 0.0 for r in rec)
            w.update(res)
        out["windows"].append(w)
        print(k, "falls back" if fell else "kept", [round(r["compression_ratio"], 3) for r in passes], flush=True)
    n_fb = sum(w["falls_back"] for w in out["windows"])
    assert 0 < n_fb < N_WINDOWS, n_fb
    json.dump(out, open(os.path.join(OUT, "e2e_fallback_golden.json"), "w"), ensure_ascii=True, indent=0)


if __name__ == "__main__":
    main()
