"""The window call of align_long (cw_align_cut_tokens) at the bench geometry: large-v3 shape, aligned synthetic weights, --items x
30 s clips resident after one mel, one row of --tokens text ids per clip, cuts allowed at every fourth token.

  one call      cw_align_cut_tokens: one forward, the STOP head, the cut on the device, the timestamp stage on the kept prefix
  two forwards  what the calls before it allow: cw_score_tokens for the token log-probabilities (no stop_logprob exists there, so
                the host picks the same cuts from the one-call run), then cw_align_tokens on every kept prefix
  head          the fused scoring head alone, plain and STOP (cw_time_score_head), interleaved, at 1024 rows

Best of --reps after one warm-up, wall time around the calls with the stream synchronised; the head by HIP events.
usage: python tools/align_long_bench.py [--dtype bf16] [--tokens 128] [--items 8] [--reps 5]"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from crisperwhisper_amd import synthetic as syn
from crisperwhisper_amd.engine import Engine
from tools.align_bench import timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16"); ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--items", type=int, default=8); ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    g, v = syn.large_v3_geometry()
    spec = syn.model_spec(g, v, n_align=15)
    B = a.items
    eng = Engine(spec, dtype=a.dtype, max_batch=B)
    for name, shape in syn.weight_shapes(g).items():
        eng.load_tensor(name, syn.weight_tensor(g, name, shape, 0, "aligned"))
    _, nf = eng.mel([syn.synth_audio(i, 480000, "noise") for i in range(B)])
    init = [v.sot, v.lang_id("en"), v.transcribe]
    rng = np.random.default_rng(0)
    ids = [np.array(init + rng.integers(0, v.eos, a.tokens).tolist() + [v.eos], np.int64) for _ in range(B)]
    # interior cuts, so that the timestamp stage of both forms runs on prefixes: one allowed n per row, spread over the row
    keep = [max(1, (a.tokens * (b + 1)) // (B + 1)) for b in range(B)]
    masks = [np.arange(a.tokens + 1) == k for k in keep]
    none = [False] * B
    out = {"dtype": a.dtype, "items": B, "tokens": a.tokens, "kept": keep}
    cut = eng.align_cut_tokens(nf, ids, 3, masks, none)[0]
    assert cut.tolist() == keep
    out["one_call_ms"], out["one_call_split_ms"] = timed(eng, lambda: eng.align_cut_tokens(nf, ids, 3, masks, none), a.reps)

    def two_forwards():
        eng.score_tokens(ids, 3)
        eng.align_tokens(nf, [np.concatenate([r[:3 + k], [v.eos]]) for r, k in zip(ids, keep)], 3)
    out["two_forwards_ms"], out["two_forwards_split_ms"] = timed(eng, two_forwards, a.reps)
    out["align_score_tokens_ms"], _ = timed(eng, lambda: eng.align_score_tokens(nf, ids, 3), a.reps)
    plain, stop = [], []
    for _ in range(3):
        plain.append(eng.time_score_head(1024, False, 10))
        stop.append(eng.time_score_head(1024, False, 10, stop=True))
    out["head_1024_ms"] = {"plain": round(min(plain), 4), "stop": round(min(stop), 4), "ratio": round(min(stop) / min(plain), 4)}
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
