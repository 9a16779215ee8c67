"""What the alignment scores (cw_set_alignment_scores) add to the timestamp stage at the bench geometry: large-v3 shape, aligned
synthetic weights, --rows x 30 s clips, one greedy decode of --tokens forced-length positions, then cw_token_timestamps on the
retained rows with the switch off and on, alternating, --reps times each after one warm-up of either.

  timestamps_off_ms / timestamps_on_ms   median (and min .. max) of the engine's CW_STAGE_TIMESTAMPS timer per call: device
                                          events around normalisation, z-score / median filter, DTW and -- when on -- the
                                          path-score kernel
  call_off_ms / call_on_ms               median wall time of the whole call (uploads, launches, the copies back), stream drained

usage: python tools/alignment_scores_bench.py [--dtype bf16] [--rows 8] [--tokens 128] [--collar 3] [--reps 20]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from crisperwhisper_amd import synthetic as syn
from crisperwhisper_amd.engine import Engine


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16"); ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--tokens", type=int, default=128); ap.add_argument("--collar", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    g, v = syn.large_v3_geometry()
    spec = syn.model_spec(g, v, n_align=15)
    B, T = a.rows, a.tokens
    eng = Engine(spec, dtype=a.dtype, max_batch=B)
    for name, shape in syn.weight_shapes(g).items():
        eng.load_tensor(name, syn.weight_tensor(g, name, shape, 0, "aligned"))
    _, nf = eng.mel([syn.synth_audio(i, 480000, "noise") for i in range(B)])
    prompt = np.tile(np.asarray([v.sot, v.lang_id("en"), v.transcribe], np.int32), (B, 1))
    eng.encode(list(range(B)), [0] * B, [3000] * B)
    _, lens, _ = eng.decode(prompt, 3 + T, min_new_tokens=T)
    L = int(lens.max()) - 1

    def call(on):
        eng.set_alignment_scores(on, a.collar)
        eng.sync()
        eng.stage_times(reset=True)
        t0 = time.perf_counter()
        ts = eng.token_timestamps(B, L, 3, nf)
        if on:
            eng.alignment_scores(B, L)
        eng.sync()
        wall = (time.perf_counter() - t0) * 1e3
        return eng.stage_times()["timestamps"][0], wall, ts

    stage, wall = {False: [], True: []}, {False: [], True: []}
    ref = None
    for r in range(a.reps + 1):
        for on in (False, True):
            s, w, ts = call(on)
            ref = ts if ref is None else ref
            assert ts.tobytes() == ref.tobytes()          # the switch changes no timestamp
            if r > 0:                                     # (the first round of either warms up)
                stage[on].append(s); wall[on].append(w)
    eng.set_alignment_scores(False)

    def stat(x):
        return {"median": round(float(np.median(x)), 4), "min": round(float(np.min(x)), 4), "max": round(float(np.max(x)), 4)}
    out = {"dtype": a.dtype, "rows": B, "tokens": T, "token_rows": L - 3, "heads": len(spec.alignment_heads), "collar": a.collar,
           "reps": a.reps, "timestamps_off_ms": stat(stage[False]), "timestamps_on_ms": stat(stage[True]),
           "call_off_ms": stat(wall[False]), "call_on_ms": stat(wall[True])}
    out["added_stage_ms"] = round(out["timestamps_on_ms"]["median"] - out["timestamps_off_ms"]["median"], 4)
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
