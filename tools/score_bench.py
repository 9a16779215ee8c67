"""Transcript scoring (cw_score_tokens) at the bench geometry: large-v3 shape, aligned synthetic weights, --items x 30 s clips
resident after one mel, --rows-per-item candidate transcripts of --tokens text ids per clip.

  score (prefill)   one cw_score_tokens call on the 16-bit engine: one encoder pass per item, one teacher-forced prefill forward
                    over every layer and the scoring head (csrc/score.hip); the split comes from the engine's stage timers
  score (loop)      the same call with cw_set_option "score_prefill" = 0: the per-position decoder step, every token forced
  head              the scoring head alone, fused and unfused (cw_time_score_head), at the call's M, 1024 and 5120 rows
  capture loop      what the library offered before cw_score_tokens: cw_decode with every token forced and cw_set_logits_capture
                    on, log-softmax and gather on the host (rows_per_item 1 only: cw_decode reads one item per row)

  --top-logprobs K  the score calls ask for the K best alternatives of every position (cw_set_score_top_logprobs), and the head
                    alone is timed in its TOPK forms (cw_time_score_head_top: k = 0, 1, 8, plain and STOP, at 1032 and 5160 rows)

"scores_sha256" digests the prefill call's log-probabilities, arg-max ids and their log-probabilities (the alternatives are not
part of it: two builds, or K = 0 and K > 0, must print the same digest).
Best of --reps after one warm-up, wall time around the call with the stream synchronised.
usage: python tools/score_bench.py [--dtype bf16] [--tokens 128] [--items 8] [--rows-per-item 1] [--reps 5] [--only-forward]
                                   [--top-logprobs 0]"""
import argparse, hashlib, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from crisperwhisper_amd import synthetic as syn
from crisperwhisper_amd.engine import Engine
from tools.align_bench import timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16"); ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--items", type=int, default=8); ap.add_argument("--rows-per-item", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only-forward", action="store_true", help="one prefill score call only (for a kernel trace)")
    ap.add_argument("--top-logprobs", type=int, default=0, help="alternatives per scored position (0 .. 8)")
    ap.add_argument("--entropy", action="store_true", help="also time the head's ENT form (cw_time_score_head_entropy) against the plain one")
    a = ap.parse_args()
    g, v = syn.large_v3_geometry()
    spec = syn.model_spec(g, v, n_align=15)
    B, K = a.items, a.rows_per_item
    eng = Engine(spec, dtype=a.dtype, max_batch=B * K)
    for name, shape in syn.weight_shapes(g).items():
        eng.load_tensor(name, syn.weight_tensor(g, name, shape, 0, "aligned"))
    eng.mel([syn.synth_audio(i, 480000, "noise") for i in range(B)])
    init = [v.sot, v.lang_id("en"), v.transcribe]
    rng = np.random.default_rng(0)
    ids = [np.array(init + rng.integers(0, v.eos, a.tokens).tolist() + [v.eos], np.int64) for _ in range(B * K)]
    top = {"top_logprobs": a.top_logprobs} if a.top_logprobs else {}      # (passed only when set: the call is today's otherwise)
    if a.only_forward:
        eng.score_tokens(ids, 3, rows_per_item=K, **top)
        eng.score_tokens(ids, 3, rows_per_item=K, **top)
        eng.sync()
        eng.close()
        return
    out = {"dtype": a.dtype, "items": B, "rows_per_item": K, "tokens": a.tokens, "scored_positions": B * K * (a.tokens + 1)}
    if top:
        out["top_logprobs"] = a.top_logprobs
    res = eng.score_tokens(ids, 3, rows_per_item=K, **top)
    out["scores_sha256"] = hashlib.sha256(b"".join(np.ascontiguousarray(x).tobytes() for part in res[:3] for x in part)).hexdigest()
    out["score_prefill_ms"], out["score_prefill_split_ms"] = timed(eng, lambda: eng.score_tokens(ids, 3, rows_per_item=K, **top), a.reps)
    eng.set_score_prefill(False)
    out["score_loop_ms"], out["score_loop_split_ms"] = timed(eng, lambda: eng.score_tokens(ids, 3, rows_per_item=K, **top),
                                                             max(1, a.reps // 2))
    eng.set_score_prefill(True)
    if K == 1:
        T = len(ids[0])
        forced = np.full((B, T), -1, np.int32)
        for b in range(B):
            forced[b, 3:] = ids[b][3:]
        prompt = np.tile(np.asarray(init, np.int32), (B, 1))

        def capture_loop():
            eng.encode(list(range(B)), [0] * B, [3000] * B)
            cap = eng.capture_logits(B, T - 3)
            eng.decode(prompt, T, 0, forced=forced)
            eng.sync()
            lg = np.asarray(cap).reshape(T - 3, B, -1).astype(np.float64)
            m = lg.max(-1, keepdims=True)
            lsm = lg - m - np.log(np.exp(lg - m).sum(-1, keepdims=True))
            res = np.take_along_axis(lsm, forced[:, 3:].T[:, :, None].astype(np.int64), -1)
            eng.stop_capture()
            return res
        out["capture_loop_ms"], out["capture_loop_split_ms"] = timed(eng, capture_loop, max(1, a.reps // 2))
    # the scoring head alone (LayerNorm + projection + log-softmax + gather) at this call's M, 1024 and 5120 rows, fused against the
    # unfused form (the same GEMM storing f32 logits [M][V], then a row-wise pass); HIP events, 10 repetitions after a warm-up
    out["head_ms"] = {str(M): {"fused": round(eng.time_score_head(M, False, 10), 3), "unfused": round(eng.time_score_head(M, True, 10), 3)}
                      for M in (B * K * (a.tokens + 1), 1024, 5120)}
    if top:                                  # the TOPK forms of the head against k = 0, timed by the same loop in this process
        out["head_top_ms"] = {str(M): {form: {str(k): round(eng.time_score_head_top(M, k, stop, 10), 3) for k in (0, 1, 8)}
                                       for form, stop in (("plain", False), ("stop", True))} for M in (1032, 5160)}
    if a.entropy:                            # [without, with] the ENT form, timed by the same loop in this process
        out["head_entropy_ms"] = {str(M): {form: {f"k{k}": [round(eng.time_score_head_top(M, k, stop, 10), 3),
                                                            round(eng.time_score_head_entropy(M, k, stop, 10), 3)] for k in (0, 8)}
                                           for form, stop in (("plain", False), ("stop", True))} for M in (1024, 5120)}
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
