"""Forced alignment (cw_align_tokens) at the bench geometry: large-v3 shape, aligned synthetic weights, 8 x 30 s clips resident
after one mel, transcripts of --tokens text ids each (decoder input = 3 init tokens + transcript, eos predicted last).

  align (prefill)   one cw_align_tokens call on the 16-bit engine: encode, one teacher-forced prefill forward that stops after the
                    last alignment layer, timestamps row by row; the split comes from the engine's stage timers
  align (loop)      the same call with cw_set_option "align_prefill" = 0: the forward through the per-position decoder step
  transcribe        cw_transcribe of the same clips, greedy, --tokens forced-length tokens (bench.py's decode)
  --heads all       cw_align_heads over every (layer, head) of the decoder with reference intervals, after the rows above: the
                    call's own split (forward, normalise, similarity, per-head timestamps; cw_align_heads_times), the similarity
                    kernel's bytes/s, and one cw_align_tokens call per head extrapolated from the measured row above

Best of --reps after one warm-up, wall time around the call with the stream synchronised.
usage: python tools/align_bench.py [--dtype bf16] [--tokens 128] [--reps 5] [--only-forward] [--heads all]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from crisperwhisper_amd import synthetic as syn
from crisperwhisper_amd.engine import Engine


def timed(eng, fn, reps):
    best, split = None, None
    for r in range(reps + 1):
        eng.sync()
        eng.stage_times(reset=True)
        t0 = time.perf_counter()
        fn()
        eng.sync()
        dt = (time.perf_counter() - t0) * 1e3
        st = eng.stage_times()
        if r > 0 and (best is None or dt < best):
            best, split = dt, {k: round(v[0], 3) for k, v in st.items() if v[1]}
    return round(best, 3), split


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16"); ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--items", type=int, default=8); ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only-forward", action="store_true", help="one prefill align call only (for a kernel trace)")
    ap.add_argument("--heads", choices=["all"], default=None, help="also time cw_align_heads over every decoder head")
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
    if a.only_forward:
        eng.align_tokens(nf, ids, 3)
        eng.sync()
        return
    out = {"dtype": a.dtype, "items": B, "tokens": a.tokens, "align_layers": sorted({l for l, _ in spec.alignment_heads}),
           "dec_layers": g.dec_layers}
    out["align_prefill_ms"], out["align_prefill_split_ms"] = timed(eng, lambda: eng.align_tokens(nf, ids, 3), a.reps)
    eng.set_align_prefill(False)
    out["align_loop_ms"], out["align_loop_split_ms"] = timed(eng, lambda: eng.align_tokens(nf, ids, 3), max(1, a.reps // 2))
    eng.set_align_prefill(True)
    out["transcribe_ms"], out["transcribe_split_ms"] = timed(
        eng, lambda: eng.transcribe(B, nf, sot=v.sot, language_token=v.lang_id("en"), task_token=v.transcribe,
                                    max_new_tokens=a.tokens, min_new_tokens=a.tokens), max(1, a.reps // 2))
    if a.heads == "all":
        heads = [[l, h] for l in range(g.dec_layers) for h in range(g.heads)]
        n_tok = [len(r) for r in ids]
        # reference intervals along the synthetic ridge (token t spoken at frame 11 t), 0.2 s long
        begin = [np.where(np.arange(n) >= 3, np.arange(n) * syn.ALIGNED_FRAMES_PER_TOKEN * 0.02, np.nan).astype(np.float32) for n in n_tok]
        end = [(b + 0.2).astype(np.float32) for b in begin]
        best = None
        for r in range(max(1, a.reps // 2) + 1):
            eng.sync()
            t0 = time.perf_counter()
            eng.align_heads(nf, ids, 3, heads, ref=(begin, end), clip_frames=200)
            eng.sync()
            dt = (time.perf_counter() - t0) * 1e3
            if r > 0 and (best is None or dt < best[0]):
                best = (dt, eng.align_heads_times())
        rows = B * len(heads) * (max(n_tok) - 1)
        out["align_heads"] = {"heads": len(heads), "total_ms": round(best[0], 3), "split_ms": {k: round(v, 3) for k, v in best[1].items()},
                              "capture_bytes": rows * 6000, "similarity_rows": rows,
                              # rows with a reference (every text token) read their n_cols = 1500 frames once
                              "similarity_kernel_TBps": round(len(heads) * sum(n - 4 for n in n_tok) * 6000 / (best[1]["similarity_kernel"] * 1e-3) / 1e12, 3),
                              # what one cw_align_tokens call per head would cost: an extrapolation from the measured
                              # 15-head call above (a single-head call runs the same encoder and, for a head in the last
                              # alignment layer, the same forward)
                              "extrapolated_single_head_calls_ms": round(out["align_prefill_ms"] * len(heads), 1)}
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
