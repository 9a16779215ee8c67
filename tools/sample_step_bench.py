"""Seeded sampling in the decode step (cw_set_sampling) and one temperature-fallback round (cw_decode_rows) at the bench
geometry: large-v3 shape, aligned synthetic weights, --rows x 30 s clips resident after one mel and one encoder pass.

  step              cw_decode over --tokens positions with eos held back (min_new_tokens), greedy and sampling at --temperature in
                    the same build: decode-stage time of the engine's timers per token step
  fallback round    encode + greedy decode of all rows + token timestamps, against the same followed by one re-decode at
                    --temperature with --redo of the rows live (the others idle through the step) and its token timestamps;
                    the stage timers carry the number of encoder passes of either call

  --token-logprobs  the step measurement once more with cw_set_token_logprobs on (the sampler also reduces the raw log-sum-exp
                    of every row and stores log_softmax(raw)[token]): step_*_logprobs_ms, off and on in the same build
  --top-logprobs K [K ...]  (with --token-logprobs) ... and once more per K with cw_set_top_logprobs(K) on top (the sampler also
                    selects the K best raw logits of every row): step_*_top<K>_ms, all in the same build and process
  --token-entropy   (with --token-logprobs) ... and once more with cw_set_token_entropy on top (the sampler also keeps the centred
                    sum of every row and stores its predictive entropy): step_*_entropy_ms, same build and process
  --sequence-bias N [N ...]  ... and once more per N with a cw_set_sequence_bias table of N entries (half single tokens, half
                    two-token sequences) whose last tokens are spread over the 16 vocabulary slices of the sampler, and once with
                    all N in one slice: step_*_bias<N>_ms / step_*_bias<N>_one_slice_ms, against the table-free figure of the same
                    process
  --no-fallback-round  leave the fallback round out

Best of --reps after one warm-up, wall time around the call with the stream synchronised.
usage: python tools/sample_step_bench.py [--dtype bf16] [--rows 8] [--tokens 128] [--temperature 0.6] [--redo 2] [--reps 5]
                                         [--token-logprobs [--top-logprobs 5 8]] [--sequence-bias 8 256] [--no-fallback-round]"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from crisperwhisper_amd import synthetic as syn
from crisperwhisper_amd.engine import Engine
from crisperwhisper_amd.generation import stream_id
from tools.align_bench import timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16"); ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--tokens", type=int, default=128); ap.add_argument("--temperature", type=float, default=0.6)
    ap.add_argument("--redo", type=int, default=2); ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--token-logprobs", action="store_true"); ap.add_argument("--no-fallback-round", action="store_true")
    ap.add_argument("--top-logprobs", type=int, nargs="+", default=[], metavar="K")
    ap.add_argument("--sequence-bias", type=int, nargs="+", default=[], metavar="N")
    ap.add_argument("--token-entropy", action="store_true")
    a = ap.parse_args()
    if a.top_logprobs and not a.token_logprobs:
        ap.error("--top-logprobs needs --token-logprobs (cw_set_top_logprobs shares its normaliser)")
    g, v = syn.large_v3_geometry()
    spec = syn.model_spec(g, v, n_align=15)
    B, T = a.rows, a.tokens
    eng = Engine(spec, dtype=a.dtype, max_batch=B)
    for name, shape in syn.weight_shapes(g).items():
        eng.load_tensor(name, syn.weight_tensor(g, name, shape, 0, "aligned"))
    _, nf = eng.mel([syn.synth_audio(i, 480000, "noise") for i in range(B)])
    prompt = np.tile(np.asarray([v.sot, v.lang_id("en"), v.transcribe], np.int32), (B, 1))
    streams = [stream_id(b, 0, 1) for b in range(B)]
    mask = np.zeros(B, np.int32); mask[:a.redo] = 1
    eng.encode(list(range(B)), [0] * B, [3000] * B)
    out = {"dtype": a.dtype, "rows": B, "tokens": T, "temperature": a.temperature, "redo": a.redo}

    def steps():
        eng.decode(prompt, 3 + T, min_new_tokens=T)
    if a.token_entropy and not a.token_logprobs:
        ap.error("--token-entropy needs --token-logprobs (cw_set_token_entropy shares its running sums)")
    variants = [("", False, 0, False)] + ([("_logprobs", True, 0, False)] if a.token_logprobs else []) + \
               [(f"_top{k}", True, k, False) for k in a.top_logprobs] + ([("_entropy", True, 0, True)] if a.token_entropy else [])
    for tag, on, k, ent in variants:
        eng.set_token_logprobs(on)
        if on:
            eng.set_top_logprobs(k)
            eng.set_token_entropy(ent)
        for name, temp in (("greedy", 0.0), ("sampling", a.temperature)):
            eng.set_sampling(temp, 1, streams)
            ms, split = timed(eng, steps, a.reps)
            out[f"step_{name}{tag}_ms"] = round(split["decode"] / T, 4)
            out[f"decode_{name}{tag}_wall_ms"] = ms
    eng.set_sampling(0.0)
    eng.set_token_logprobs(False)
    V = spec.vocab_size
    per = ((((V + 3) // 4) + 15) // 16) * 4                          # columns per sampler slice
    for n in a.sequence_bias:
        for tag, last in ((f"_bias{n}", lambda i: (i * V) // n + 5), (f"_bias{n}_one_slice", lambda i: 3 * per + i)):
            table = [((last(i),) if i % 2 == 0 else (int(v.transcribe), last(i)), 0.25 + (i % 5)) for i in range(n)]
            eng.set_sequence_bias(table)
            for name, temp in (("greedy", 0.0), ("sampling", a.temperature)):
                eng.set_sampling(temp, 1, streams)
                ms, split = timed(eng, steps, a.reps)
                out[f"step_{name}{tag}_ms"] = round(split["decode"] / T, 4)
                out[f"decode_{name}{tag}_wall_ms"] = ms
    eng.set_sampling(0.0)
    eng.set_sequence_bias(None)
    if a.no_fallback_round:
        print(json.dumps(out))
        eng.close()
        return

    def round_(redo):
        def fn():
            eng.encode(list(range(B)), [0] * B, [3000] * B)
            _, lens, _ = eng.decode(prompt, 3 + T, min_new_tokens=T)
            eng.token_timestamps(B, int(lens.max()) - 1, 3, nf)
            if redo:
                eng.set_sampling(a.temperature, 1, streams)
                _, lens, _ = eng.decode(prompt, 3 + T, min_new_tokens=T, row_active=mask)
                eng.token_timestamps(B, int(lens.max()) - 1, 3, nf)
                eng.set_sampling(0.0)
        return fn
    for name, redo in (("no_fallback", False), ("one_fallback_round", True)):
        ms, split = timed(eng, round_(redo), a.reps)
        eng.stage_times(reset=True)
        round_(redo)()
        eng.sync()
        out[name] = {"wall_ms": ms, "split_ms": split, "encoder_passes": eng.stage_times()["encoder"][1]}
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
