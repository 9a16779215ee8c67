"""Time of language detection at 8 and 64 rows on the bf16 engine at large-v3 geometry: cw_detect_language
against the route it replaces, cw_decode(max_length 2) + cw_get_logits + host arg-max, which stays callable.  The routes
alternate in one process, the stream is drained before and after every repetition, 5 warm-up repetitions are discarded, the
median of 25 is reported with the bytes each route copies back; the languages and the position-0 logits of the two routes are
asserted equal first.  python tools/langid_bench.py"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from crisperwhisper_amd import synthetic as syn          # noqa: E402
from crisperwhisper_amd.engine import Engine             # noqa: E402

WARM, REPS = 5, 25
g, v = syn.large_v3_geometry()
spec = syn.model_spec(g, v)
t0 = time.perf_counter()
eng = Engine(spec, dtype="bf16", max_batch=64)
for name, shape in syn.weight_shapes(g).items():
    eng.load_tensor(name, syn.weight_tensor(g, name, shape, 0, "iid"))
print(f"weights loaded in {time.perf_counter() - t0:.1f} s", flush=True)
V = spec.vocab_size
ids = (spec.decoder_start_token_id + 1 + np.arange(100)).astype(np.int32)      # 100 candidates, as large-v3 has
ids = ids[ids < V]
res = {}
for nb in (8, 64):
    clips = [syn.synth_audio(200 + b, 30 * 16000, ("noise", "chirp", "mixed")[b % 3]) for b in range(nb)]
    eng.mel(clips)
    eng.encode(list(range(nb)), [0] * nb, [3000] * nb)
    prompt = np.full((nb, 1), spec.decoder_start_token_id, np.int32)

    def old():
        eng.decode(prompt, max_length=2)
        lg = eng.last_logits(nb)
        return ids[np.argmax(lg[:, ids], axis=-1)], lg

    def old_forward_only():
        eng.decode(prompt, max_length=2)
        eng.sync()

    def new():
        return eng.detect_language(nb, ids, no_speech=False)

    def new_ns():
        return eng.detect_language(nb, ids, no_speech=True)

    a, lg_old = old()
    b = new()
    assert a.tolist() == b[0].tolist(), "the two routes disagree"
    assert eng.last_logits(nb).tobytes() == lg_old.tobytes(), "position-0 logits differ"
    routes = {"old": old, "old_forward_only": old_forward_only, "new": new, "new_with_no_speech": new_ns}
    times = {k: [] for k in routes}
    for rep in range(WARM + REPS):
        for k, fn in routes.items():
            eng.sync()
            t = time.perf_counter()
            fn()
            eng.sync()
            if rep >= WARM:
                times[k].append((time.perf_counter() - t) * 1e3)
    res[nb] = {k: {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)} for k, t in times.items()}
    res[nb]["bytes_old"] = nb * V * 4
    res[nb]["bytes_new"] = nb * (len(ids) + 2) * 4
    print(nb, json.dumps(res[nb]), flush=True)

print(json.dumps(res))
eng.close()
