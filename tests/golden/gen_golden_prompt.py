"""Goldens for ``generate_kwargs={"prompt_ids": ...}``: the reference pipeline call through the installed transformers 5.15.0
(CPU, fp32) with ``prompt_ids = tokenizer.get_prompt_ids(text, return_tensors="pt")``, i.e. decoder input
``<|startofprev|> p1 .. pk <|startoftranscript|> <|lang|> <|task|>`` in every generate call of every 30 s chunk
(generation_whisper.py:1909-1913; condition_on_prev_tokens stays False).

Tiny geometry (i.i.d. random weights, like gen_golden_beam.py): prompt lengths 2, 17, 70 (the first generated step then
attends to more than 64 keys) and 440 (3 + 440 + 5 = the 448 limit), greedy and 5 beams, 20 s and 70 s clips, one call with
language detection.  Recorded per scenario: the prompt ids, the pipeline's text and word chunks, and for every generate call
the sequences and the per-item token timestamps of its segments.

Bench geometry (``--bench``; aligned weights as gen_golden_bench.py, the 8 bench clips, one clip per pipeline call): a 32-token
prompt with max_new_tokens = min_new_tokens = 96.  The aligned decoder ridge sits at frame 11 * position, so 11 * (3 + 32 + 96)
= 1441 stays below the 1500 encoder frames.  ~20 CPU minutes.

    python -m tests.golden.gen_golden_prompt            -> tests/golden/e2e_prompt_golden.json / .npz
    python -m tests.golden.gen_golden_prompt --bench    -> tests/golden/e2e_bench_prompt_golden.json"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from crisperwhisper_amd import synthetic as syn
from tests.golden import hf_synth as H
from tests.golden.gen_golden import build_tiny

OUT = os.path.dirname(os.path.abspath(__file__))
EN = {"language": "<|en|>", "task": "transcribe"}
# get_prompt_ids on the byte-level synthetic tokenizer: <|startofprev|> + one token per byte of " " + text.strip()
_TEXT = ("Dr. Nguyen prescribed paracetamol 500 mg and cetirizine; verbatim: um, uh, hmm. "
         "Patient reports tinnitus, vertigo and photophobia since Tuesday. ")


def prompt_text(n_tokens: int) -> str:
    """A prompt text whose get_prompt_ids is exactly ``n_tokens`` long (n_tokens >= 2)."""
    n = n_tokens - 2
    s = (_TEXT * (1 + n // len(_TEXT)))[:n]
    if s.endswith(" ") or s.startswith(" "):            # strip() would shorten it
        s = s[:-1] + "x" if s.endswith(" ") else "x" + s[1:]
    return s


SCENARIOS = {
    # name: (audio kind, seconds, seed, batch_size, prompt tokens, generate kwargs besides prompt_ids)
    "p2_greedy_noise20_b1_n40": ("noise", 20, 41, 1, 2, {**EN, "num_beams": 1, "max_new_tokens": 40}),
    "p17_greedy_mixed70_b2_n40": ("mixed", 70, 42, 2, 17, {**EN, "num_beams": 1, "max_new_tokens": 40}),
    "p70_greedy_noise20_b1_n32": ("noise", 20, 43, 1, 70, {**EN, "num_beams": 1, "max_new_tokens": 32}),
    "p25_greedy_noise20_b1_free": ("noise", 20, 44, 1, 25, {**EN, "num_beams": 1}),
    "p17_detect_noise20_b1_n24": ("noise", 20, 45, 1, 17, {"num_beams": 1, "max_new_tokens": 24}),
    "p440_greedy_noise20_b1_n5": ("noise", 20, 46, 1, 440, {**EN, "num_beams": 1, "max_new_tokens": 5}),
    "p17_beam5_noise20_b1_n24": ("noise", 20, 47, 1, 17, {**EN, "num_beams": 5, "max_new_tokens": 24}),
    "p70_beam5_mixed70_b2_n24": ("mixed", 70, 48, 2, 70, {**EN, "num_beams": 5, "max_new_tokens": 24}),
    "p440_beam5_noise20_b1_n5": ("noise", 20, 49, 1, 440, {**EN, "num_beams": 5, "max_new_tokens": 5}),
}

BENCH_CLIPS, BENCH_PROMPT, BENCH_TOK = 8, 32, 96
BENCH_KW = {**EN, "num_beams": 1, "max_new_tokens": BENCH_TOK, "min_new_tokens": BENCH_TOK}


def gen_tiny():
    torch.set_num_threads(2)
    torch.manual_seed(0)
    g, v, W, model = build_tiny()
    tok = H.build_tokenizer(v)
    fe = H.build_feature_extractor(g)
    meta, arrays = {}, {}
    for name, (kind, secs, seed, bs, n_p, gk) in SCENARIOS.items():
        pids = tok.get_prompt_ids(prompt_text(n_p), return_tensors="pt")
        assert len(pids) == n_p and int(pids[0]) == v.startofprev, (name, len(pids))
        x = syn.synth_audio(seed, int(round(secs * 16000)), kind)
        pipe = H.build_pipeline(model, tok, fe, batch_size=bs)
        calls = []
        orig = model.generate

        def spy(*a, **k):
            out = orig(*a, **k)
            calls.append(out)
            return out

        model.generate = spy
        try:
            res = pipe(x.copy(), generate_kwargs={**gk, "prompt_ids": pids})
        finally:
            model.generate = orig
        meta[name] = {"kind": kind, "secs": secs, "seed": seed, "batch_size": bs, "generate_kwargs": gk,
                      "prompt_text": prompt_text(n_p), "prompt_ids": [int(t) for t in pids], "text": res["text"],
                      "chunks": [{"text": c["text"], "timestamp": list(c["timestamp"])} for c in res["chunks"]],
                      "n_generate_calls": len(calls)}
        for ci, out in enumerate(calls):
            arrays[f"{name}/call{ci}/sequences"] = out["sequences"].numpy().astype(np.int64)
            for bi, segs in enumerate(out["segments"]):
                arrays[f"{name}/call{ci}/tts{bi}"] = (torch.cat([s["token_timestamps"] for s in segs]).numpy().astype(np.float32)
                                                      if segs else np.zeros(0, np.float32))
        print(name, len(res["chunks"]), "words", len(calls), "generate calls", res["text"][:50].encode(), flush=True)
    json.dump(meta, open(os.path.join(OUT, "e2e_prompt_golden.json"), "w"), ensure_ascii=True, indent=0)
    np.savez_compressed(os.path.join(OUT, "e2e_prompt_golden.npz"), **arrays)


def gen_bench():
    torch.set_num_threads(os.cpu_count())
    g, v = syn.large_v3_geometry()
    t0 = time.time()
    model = H.build_model(g, v, n_align=15)
    sd = {n: torch.from_numpy(syn.weight_tensor(g, n, shape, 0, "aligned")) for n, shape in syn.weight_shapes(g).items()}
    sd["proj_out.weight"] = sd["model.decoder.embed_tokens.weight"]
    model.load_state_dict(sd, strict=True)
    del sd
    model.generation_config.alignment_heads = syn.alignment_heads(g, 15)
    tok = H.build_tokenizer(v)
    fe = H.build_feature_extractor(g)
    print("model ready in %.0f s" % (time.time() - t0), flush=True)
    pipe = H.build_pipeline(model, tok, fe, batch_size=1)
    pids = tok.get_prompt_ids(prompt_text(BENCH_PROMPT), return_tensors="pt")
    assert len(pids) == BENCH_PROMPT
    passes = []
    orig = model._extract_token_timestamps

    def spy(generate_outputs, alignment_heads, time_precision=0.02, num_frames=None, num_input_ids=None):
        ts = orig(generate_outputs, alignment_heads, time_precision=time_precision, num_frames=num_frames, num_input_ids=num_input_ids)
        nf = num_frames
        if nf is not None and not isinstance(nf, int):
            nf = [int(x) for x in np.asarray(nf).reshape(-1)]
        passes.append({"sequences": generate_outputs["sequences"].numpy().astype(np.int64).tolist(),
                       "token_timestamps": ts.numpy().astype(np.float64).round(4).tolist(),
                       "num_frames": nf, "num_input_ids": int(num_input_ids)})
        return ts

    model._extract_token_timestamps = spy
    path = os.path.join(OUT, "e2e_bench_prompt_golden.json")
    meta = {"weights": "aligned", "weight_seed": 0, "generate_kwargs": BENCH_KW, "prompt_text": prompt_text(BENCH_PROMPT),
            "prompt_ids": [int(t) for t in pids], "clips": []}
    for seed in range(BENCH_CLIPS):
        x = syn.synth_audio(seed, 480000, "noise")
        passes.clear()
        t0 = time.time()
        res = pipe(x.copy(), generate_kwargs={**BENCH_KW, "prompt_ids": pids})
        print("clip", seed, "%.0f s" % (time.time() - t0), len(res["chunks"]), "words", len(passes), "passes", flush=True)
        meta["clips"].append({"seed": seed, "kind": "noise", "secs": 30, "text": res["text"],
                              "chunks": [{"text": c["text"], "timestamp": list(c["timestamp"])} for c in res["chunks"]],
                              "passes": [dict(p) for p in passes]})
        json.dump(meta, open(path, "w"), ensure_ascii=True, indent=0)


if __name__ == "__main__":
    if "--bench" in sys.argv[1:]:
        gen_bench()
    else:
        gen_tiny()
