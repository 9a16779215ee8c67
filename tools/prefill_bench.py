"""Decoder prompt prefill (csrc/prefill.hip) against the per-position loop (cw_set_option "prompt_prefill" = 0): cost of
generate_kwargs={"prompt_ids": ...} at the bench geometry (large-v3 shape, aligned synthetic weights, 8 x 30 s clips
encoded once).  For each prompt length P (decoder input = P prompt ids + 3 init tokens):

  prompt phase   the decoder forwards over the P forward-only input positions: a decode call with one generated token from the
                 prompted input minus the same call from the 3 init tokens alone (greedy, 8 rows), and cw_beam_begin from the
                 prompted input minus from the init tokens (8 items x 5 beams = 40 rows).
  per batch      one generate pass of 128 forced-length tokens, prompted against unprompted (greedy, 8 rows).

Best of --reps after one warm-up.  usage: python tools/prefill_bench.py [--dtype bf16] [--prompts 32,64,200] [--reps 3]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from crisperwhisper_amd import synthetic as syn
from crisperwhisper_amd.engine import Engine


def best(fn, reps, sync):
    ts = []
    for _ in range(reps + 1):
        sync(); t0 = time.perf_counter()
        fn()
        sync(); ts.append(time.perf_counter() - t0)
    return min(ts[1:]) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16"); ap.add_argument("--prompts", default="32,64,200")
    ap.add_argument("--reps", type=int, default=3); ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--items", type=int, default=8); ap.add_argument("--beams", type=int, default=5)
    a = ap.parse_args()
    g, v = syn.large_v3_geometry()
    spec = syn.model_spec(g, v, n_align=15)
    B, K = a.items, a.beams
    eng = Engine(spec, dtype=a.dtype, max_batch=B * K)
    for name, shape in syn.weight_shapes(g).items():
        eng.load_tensor(name, syn.weight_tensor(g, name, shape, 0, "aligned"))
    eng.mel([syn.synth_audio(i, 480000, "noise") for i in range(B)])
    eng.encode(list(range(B)), [0] * B, [3000] * B)
    init = [v.sot, v.lang_id("en"), v.transcribe]
    rng = np.random.default_rng(0)
    rows = []

    def launches_bytes_flops(P):
        """Prefill launches per layer and its algorithmic bytes / FLOPs at rows B (greedy) for P forward-only positions."""
        D, F, L, H = g.d_model, g.ffn, g.dec_layers, g.heads
        M = B * P
        w_bytes = L * 2 * (3 * D * D + D * D + D * D + D * D + 2 * D * F)
        kv_bytes = (L - 1) * 2 * 2 * B * 1500 * D
        act = L * 2 * M * (8 * D + 2 * F) + 4 * M * D * 3 * L
        flops = L * 2 * M * (4 * D * D + 2 * D * D + 2 * D * F) + (L - 1) * 2 * 2 * B * H * 64 * (P * P / 2 + P * 1500)
        return {"launches_per_layer": 11, "launches_last_layer": 2, "algo_bytes_GB": round((w_bytes + kv_bytes + act) / 1e9, 3),
                "algo_TFLOP": round(flops / 1e12, 4)}

    def run(prefix):
        pr = np.tile(np.array(prefix + init, np.int32), (B, 1))
        n = pr.shape[1]
        eng.set_prompt_prefix(len(prefix))
        first = best(lambda: eng.decode(pr, max_length=n + 1, min_new_tokens=1), a.reps, eng.sync)
        beam = best(lambda: eng.beam_begin(pr, K, n + 1, 0), a.reps, eng.sync)
        full = best(lambda: eng.decode(pr, max_length=n + a.tokens, min_new_tokens=a.tokens), a.reps, eng.sync)
        eng.set_prompt_prefix(0)
        return first, beam, full

    f0, b0, e0 = run([])
    for P in [int(p) for p in a.prompts.split(",")]:
        prefix = [v.startofprev] + [int(t) for t in rng.integers(32, 127, P - 1)]
        r = {"dtype": a.dtype, "prompt_tokens": P, "items": B, "beams": K, "tokens": a.tokens, "batch_ms_unprompted": round(e0, 3)}
        for tag, on in (("prefill", True), ("loop", False)):
            eng.set_prompt_prefill(on)
            f, b, e = run(prefix)
            r.update({f"prompt_phase_ms_greedy_{tag}": round(f - f0, 3), f"prompt_phase_ms_beam_{tag}": round(b - b0, 3),
                      f"batch_ms_prompted_{tag}": round(e, 3), f"batch_overhead_pct_{tag}": round(100.0 * (e - e0) / e0, 2)})
        eng.set_prompt_prefill(True)
        r.update(launches_bytes_flops(P + 2))          # P prompt ids + 3 init tokens: P + 2 forward-only positions
        rows.append(r)
        print(json.dumps(r), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
