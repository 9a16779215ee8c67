#!/usr/bin/env python
"""bench.py -- BASELINE.json metric on MI355X: RTF + aligned words/s for the full CrisperWhisper path
(log-mel -> Whisper large-v3-geometry encoder/decoder -> alignment-head capture -> z-score/median/DTW
-> word collation -> pause split) on batches of 30 s synthetic 16 kHz clips.

    python bench.py --gpus 1 --steps K --warmup W          (N=1)
    python bench.py ... --dump-outputs DIR                 (+ the last timed step's results as DIR/*.npy: dump_outputs)
    python bench.py ... --full                             (+ everything beyond the headline: see below)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

One "step" = one pass of the whole path over one batch of B x 30 s clips per GPU (weak scaling: every
rank processes its own B clips; the only collective is the all-gather of per-chunk word records).
PCM is resident in HBM before the timed region (PCIe-inclusive rate: see DESIGN.md).  Weights are
seeded random tensors of the large-v3 geometry (no checkpoint is available offline): data="synthetic".

A plain run does what the headline needs: set up, warm up, time the steps, dump the outputs if asked, print the line.
--full adds what takes work of its own after the timed steps: the parity check of the timed output against the committed
transformers goldens (and exit status 3 when it fails), the per-launch roofline (cw_time_decode_stage / cw_time_kernel runs),
the BASELINE configs[2] long-form and configs[3] batch-64 legs and the CPU reference leg; --no-longform, --no-config3,
--no-cpu-baseline, --cpu-* and --kernel-iters select within it.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


PMC_FILE = "r06_pmc_traffic_B8.json"     # latest committed PMC pass (tools/ab/run_gpu_pmc.sh + profiles/summarize_pmc.py)


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=8, help="30 s chunks in flight per GPU (BASELINE config[1]: 8)")
    ap.add_argument("--tokens", type=int, default=128, help="generated tokens per chunk (SURVEY.md 8d)")
    ap.add_argument("--geometry", default="large-v3", choices=["large-v3", "tiny"])
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16", "f32"])
    ap.add_argument("--weights", default="aligned", choices=["aligned", "iid"],
                    help="seeded synthetic weights: 'aligned' = random tensors whose alignment heads are peaked and monotone like a "
                         "trained checkpoint's (crisperwhisper_amd/synthetic.py); the run is then checked word for word against the "
                         "committed transformers output for the same clips (tests/golden/e2e_bench_golden.json)")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beyond the headline figure: parity against the committed transformers goldens, the "
                         "per-launch roofline, the configs[2] long-form and configs[3] legs and the CPU reference leg")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-tokens", type=int, default=12)
    ap.add_argument("--cpu-threads", type=int, default=0, help="torch threads of the reference leg; 0 = calibrated per stage on "
                    "the host (oracle/hf_reference.py:calibrate_threads: GEMM-shaped encoder vs M=1 decoder steps)")
    ap.add_argument("--cpu-timeout", type=int, default=360, help="hard limit (s) of the reference leg (two samples of the clip)")
    ap.add_argument("--cpu-port", action="store_true", help="also time the numpy/C oracle (kind=port) beside the reference")
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--cross-kv", default="bf16", choices=["bf16", "fp8"],
                    help="fp8: opt-in e4m3 cross-attention cache (accuracy-gated mode, not the headline)")
    ap.add_argument("--encoder-gemm", default="bf16", choices=["bf16", "fp8"],
                    help="fp8: the encoder's qkv / fc1 / fc2 and the cross-K/V projections as e4m3 MFMA GEMMs (opt-in mode, BASELINE "
                         "configs[3]; accuracy-gated, not the parity path)")
    ap.add_argument("--no-rccl", action="store_true", help="N=1 only: do not create the one-rank RCCL communicator")
    ap.add_argument("--no-longform", action="store_true", help="skip the BASELINE configs[2] leg (600 s recording sharded over the ranks)")
    ap.add_argument("--longform-seconds", type=int, default=600)
    ap.add_argument("--no-config3", action="store_true", help="skip the BASELINE configs[3] leg (batch 64, bf16 and the opt-in fp8 mode, 2 steps each; N = 1 only)")
    ap.add_argument("--num-beams", type=int, default=1,
                    help="beam search width (default 1 = greedy, the BASELINE configuration; 5 = what the literal reference call "
                         "decodes with under transformers 5.x); the engine is provisioned with batch x beams decoder rows")
    ap.add_argument("--contexts", type=int, default=1,
                    help="independent engine contexts per GPU, each with its own batch of --batch chunks, driven by "
                         "host threads (the decode step is latency-bound, so a second batch fills idle CUs); "
                         "default 1 = the BASELINE configuration")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (rank 0; see dump_outputs)")
    a = ap.parse_args(argv)
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    if a.warmup < 0:
        ap.error("--warmup must not be negative")
    return a


DUMP_BYTES_MAX = 64 << 20


def dump_outputs(path, records, local_outs, pad_token_id, max_bytes=DUMP_BYTES_MAX):
    """Write the last timed step's results as float32 / float64 .npy files under `path`, one row per chunk, rows in chunk order:
    chunk_index [N] (the chunk's seed), word_counts [N], word_timestamps [N, W, 2] (start, end in s, after the pause split; NaN
    pad), word_text_utf8 [N, T] (the words' UTF-8 joined by 0x00; -1 pad), sequences [N, L] (generated token ids; pad_token_id
    pad) and token_timestamps [N, L] (s; NaN pad).  `records` = the gathered word records of every rank; `local_outs` = chunk
    index -> (token ids, token timestamps) of this rank's chunks (rows of other ranks' chunks stay NaN in the last two).
    Over `max_bytes` in all, a fixed seeded sample of the rows is written."""
    from crisperwhisper_amd import dist
    recs = sorted((dist.unpack_words(r) for r in records), key=lambda r: r[0])
    n = len(recs)
    n_words = max((len(w) for _, w in recs), default=0)
    blobs = [b"\x00".join(w_["text"].encode("utf-8") for w_ in w) for _, w in recs]
    n_len = max((max(len(t), len(s)) for t, s in local_outs.values()), default=0)
    arrays = {"chunk_index": np.array([i for i, _ in recs], dtype=np.float64),
              "word_counts": np.array([len(w) for _, w in recs], dtype=np.float64),
              "word_timestamps": np.full((n, n_words, 2), np.nan, dtype=np.float64),
              "word_text_utf8": np.full((n, max((len(b) for b in blobs), default=0)), -1.0, dtype=np.float32),
              "sequences": np.full((n, n_len), np.nan, dtype=np.float64),
              "token_timestamps": np.full((n, n_len), np.nan, dtype=np.float32)}
    for row, ((idx, words), blob) in enumerate(zip(recs, blobs)):
        if words:
            arrays["word_timestamps"][row, :len(words)] = [w_["timestamp"] for w_ in words]
        arrays["word_text_utf8"][row, :len(blob)] = np.frombuffer(blob, dtype=np.uint8)
        if idx in local_outs:
            toks, ts = local_outs[idx]
            arrays["sequences"][row] = pad_token_id
            arrays["sequences"][row, :len(toks)] = toks
            arrays["token_timestamps"][row, :len(ts)] = ts
    total = sum(x.nbytes for x in arrays.values())
    if total > max_bytes:
        keep = np.sort(np.random.default_rng(0).choice(n, max(1, n * max_bytes // total), replace=False))
        arrays = {k: x[keep] for k, x in arrays.items()}
    os.makedirs(path, exist_ok=True)
    for k, x in arrays.items():
        np.save(os.path.join(path, f"{k}.npy"), x)
    return arrays


def cpu_baseline(g, v, spec, weights, n_tok_gpu, words_per_chunk, cpu_tokens):
    """Reference algorithm on the host cores: the numpy/C oracle (kind="port") on a bounded sample --
    one 30 s clip, `cpu_tokens` new tokens -- extrapolated to the GPU workload's token count."""
    from oracle import generate as OG
    from oracle import mel as OM
    from oracle import timestamps as OT
    from oracle.model import WhisperOracle
    from crisperwhisper_amd import synthetic as syn
    x = syn.synth_audio(0, 480000, "noise")
    t0 = time.perf_counter()
    feats = OM.log_mel(x[None], g.n_mels)
    t_mel = time.perf_counter() - t0
    orc = WhisperOracle(weights, g)
    t0 = time.perf_counter()
    enc = orc.encode(feats)
    t_enc = time.perf_counter() - t0
    ospec = OG.GenSpec(eos=v.eos, pad=v.eos, sot=v.sot, no_timestamps=v.notimestamps, lang_to_id=spec.lang_to_id,
                       task_to_id=spec.task_to_id, alignment_heads=[list(h) for h in spec.alignment_heads],
                       suppress=v.suppress_tokens(), begin_suppress=v.begin_suppress_tokens(),
                       max_initial_timestamp_index=50, max_length=g.max_target_positions,
                       median_filter_width=g.median_filter_width)
    prompt = np.array([[v.sot, v.lang_id("en"), v.transcribe]], dtype=np.int64)
    t0 = time.perf_counter()
    seqs, weights_rows = OG.greedy(orc, ospec, enc, prompt, begin_index=3, max_new_tokens=cpu_tokens, min_new_tokens=cpu_tokens)
    t_dec = time.perf_counter() - t0
    t0 = time.perf_counter()
    # alignment stage on the full-size matrix (N = n_tok_gpu rows) so it is not under-counted
    reps = int(np.ceil((n_tok_gpu + 2) / weights_rows.shape[2]))
    wfull = np.tile(weights_rows, (1, 1, reps, 1))[:, :, :n_tok_gpu + 2]
    OT.extract_token_timestamps(wfull, np.array([3000]), 3, g.median_filter_width)
    t_ts = time.perf_counter() - t0
    per_step = t_dec / (cpu_tokens + 2)               # prompt positions are fed too
    try:                                              # threads the BLAS behind numpy actually runs with
        from threadpoolctl import threadpool_info
        blas_threads = max([i.get("num_threads", 1) for i in threadpool_info() if i.get("user_api") == "blas"] or [1])
    except Exception:
        blas_threads = os.cpu_count()
    total = t_mel + t_enc + per_step * (n_tok_gpu + 2) + t_ts
    return {"value": words_per_chunk / total, "unit": "aligned words/s", "cores": blas_threads, "host_cpus": os.cpu_count(),
            "kind": "port",
            "sample": f"1 x 30 s clip on numpy/C oracle (fp32): mel {t_mel:.2f}s + encoder {t_enc:.2f}s + "
                      f"{cpu_tokens}+2 decoder steps {t_dec:.2f}s + alignment(N={n_tok_gpu}) {t_ts:.2f}s, decoder "
                      f"extrapolated to {n_tok_gpu} tokens -> {total:.1f}s per chunk (RTF {total / 30:.3f})",
            "rtf": total / 30.0}


def cpu_reference(geometry, n_tok, threads, timeout_s, style="aligned"):
    """The reference's own path on the host cores (kind="reference"): transformers' pipeline called exactly as
    REF/transcribe.py:21-33 does (CPU, fp32, batch_size=1, word timestamps) + the REF/utils.py pause split, on one 30 s
    clip of the bench workload (clip 0) with the bench's token count and the same seeded weights as the GPU engine.
    Runs as a subprocess (oracle/hf_reference.py) under a hard timeout so that a slow host cannot lose the GPU line."""
    import subprocess
    cmd = [sys.executable, "-m", "oracle.hf_reference", "--geometry", geometry, "--tokens", str(n_tok), "--threads", str(threads), "--style", style,
           "--repeats", "2"]
    try:
        p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=timeout_s)
    except subprocess.TimeoutExpired:
        return {"value": None, "unit": "aligned words/s", "cores": threads, "host_cpus": os.cpu_count(), "kind": "reference",
                "sample": f"transformers pipeline on the host did not finish one 30 s clip ({n_tok} tokens, {threads} threads) within {timeout_s} s"}
    line = [l for l in p.stdout.splitlines() if l.startswith("REFJSON ")]
    if p.returncode != 0 or not line:
        return {"value": None, "unit": "aligned words/s", "cores": threads, "host_cpus": os.cpu_count(), "kind": "reference",
                "sample": f"failed rc={p.returncode}: {p.stderr[-300:]}"}
    r = json.loads(line[-1][8:])
    st = r["stage_s"]
    return {"value": r["words"] / r["wall_s"], "unit": "aligned words/s", "cores": r["threads"], "host_cpus": r["host_cpus"],
            "cpu_model": r["cpu_model"], "kind": "reference", "rtf": r["wall_s"] / r["audio_s"],
            # every sample of the same clip (value = the fastest): host timings of this leg moved by 20 % between rounds
            "samples_aligned_words_per_s": [r["words"] / w for w in r.get("wall_s_samples", [r["wall_s"]])],
            # seconds per probe for every torch thread count tried on this host ("gemm" = encoder-shaped, "gemv" = one decoder
            # forward's op chain); the reference leg runs each stage at its fastest count, not at os.cpu_count()
            "thread_calibration": r.get("thread_calibration") or None,
            "sample": f"1 x 30 s clip (bench clip 0) through transformers.pipeline('automatic-speech-recognition', chunk_length_s=30, "
                      f"batch_size=1, return_timestamps='word', fp32, device='cpu') + adjust_pauses, greedy, {n_tok} tokens per generate "
                      f"call, torch threads {r.get('threads_encoder')} (encoder) / {r.get('threads_decoder')} (decoder), calibrated, of {r['host_cpus']} host CPUs: {r['wall_s']:.1f} s wall for {r['words']} words (encoder {st['encoder']:.1f} s in "
                      f"{r['stage_calls']['encoder']} passes, decoder {st['decoder']:.1f} s in {r['stage_calls']['decoder']} forwards, "
                      f"token timestamps {st['token_timestamps']:.1f} s); model build {r['build_s']:.1f} s not counted"}


def load_beam_goldens(tokens, weights, num_beams):
    """seed -> reference clip record for `--num-beams 5` (what the literal reference call decodes with under transformers 5.x):
    tests/golden/e2e_bench_beam128_golden.json (gen_golden_bench_beam.py with CW_GOLD_CLIPS=8 CW_GOLD_TOKENS=128: the 8 bench clips,
    5 beams, 128 forced-length tokens per generate call, transformers CPU fp32)."""
    path = os.path.join(ROOT, "tests", "golden", "e2e_bench_beam128_golden.json")
    if not os.path.exists(path):
        return {}
    gold = json.load(open(path))
    gk = gold["generate_kwargs"]
    if gk["max_new_tokens"] != tokens or gk["num_beams"] != num_beams or gold.get("weights") != weights or gold.get("weight_seed", 0) != 0:
        return {}
    return {int(c["seed"]): c for c in gold["clips"]}


def load_bench_goldens(tokens, weights):
    """seed -> reference clip record (text, word chunks) of the transformers pipeline run on the bench clips: seeds 0..7 from
    tests/golden/e2e_bench_golden.json (gen_golden_bench.py), seeds 8..63 from e2e_bench_b64_golden.json (gen_golden_bench64.py).
    Empty when the goldens do not describe this run (other token count / weight family)."""
    out = {}
    for name in ("e2e_bench_golden.json", "e2e_bench_b64_golden.json"):
        path = os.path.join(ROOT, "tests", "golden", name)
        if not os.path.exists(path):
            continue
        gold = json.load(open(path))
        if gold["generate_kwargs"]["max_new_tokens"] != tokens or gold.get("weights") != weights or gold.get("weight_seed", 0) != 0:
            continue
        for c in gold["clips"]:
            if c.get("kind", "noise") == "noise" and c.get("secs", 30) == 30:
                out.setdefault(int(c["seed"]), c)
    return out


def words_match(mine_text, mine_chunks, ref):
    """(text identical and same word count, words identical and within 20 ms, words compared)"""
    if mine_text != ref["text"] or len(mine_chunks) != len(ref["chunks"]):
        return False, 0, 0
    ok = sum(int(wa["text"] == wb["text"] and all(abs(x - y) <= 0.02 + 1e-9 for x, y in zip(wa["timestamp"], wb["timestamp"])))
             for wa, wb in zip(mine_chunks, ref["chunks"]))
    return True, ok, len(ref["chunks"])


def config3_leg(a, dev, g, v, spec):
    """BASELINE configs[3] (throughput ceiling): batch = 64 x 30 s on one GPU, the same step as the headline -- in the parity dtype
    (bf16), in the fp8 mode that still reproduces every reference clip (fc1 as an e4m3 MFMA GEMM + e4m3 cross-attention cache:
    the largest such subset, profiles/r04_fp8_sweep.txt) and with every encoder / cross-K/V GEMM in e4m3 (fp8_all: accuracy-gated,
    not word for word).  1 warm-up + 2 timed steps each; every clip of the batch is checked against its reference record
    (tests/golden/gen_golden_bench.py + gen_golden_bench64.py)."""
    from crisperwhisper_amd import collate, generation, synthetic as syn
    from crisperwhisper_amd.engine import Engine
    B3 = 64
    vocab = collate.Vocabulary.from_synthetic(v)
    gold = load_bench_goldens(a.tokens, a.weights)
    clips = [syn.synth_audio(i, 480000, "noise") for i in range(B3)]
    out = {"workload": f"BASELINE configs[3]: batch={B3} x 30 s, {a.tokens} tokens/chunk, 1 warm-up + 2 timed steps per mode", "modes": {}}
    # fp8 = the largest e4m3 subset that reproduces every reference clip (profiles/r04_fp8_sweep.txt): fc1 as an e4m3 MFMA GEMM +
    # the e4m3 cross-attention cache; fp8_all = every encoder / cross-K/V GEMM in e4m3 as well (accuracy-gated, not word for word)
    for mode in ("bf16", "fp8", "fp8_all"):
        eng = Engine(spec, dtype=a.dtype, max_batch=B3, device=dev, cross_kv_dtype="fp8" if mode != "bf16" else None)
        try:
            for name, shape in syn.weight_shapes(g).items():
                eng.load_tensor(name, syn.weight_tensor(g, name, shape, 0, a.weights))
            if mode != "bf16":
                eng.check_weights()
                eng.set_encoder_gemm_fp8(True if mode == "fp8_all" else "fc1")
            nf = eng.upload_pcm(clips)

            def one():
                eng.mel_resident(B3)
                return generation.generate(eng, B3, nf, language="<|en|>", task="transcribe", max_new_tokens=a.tokens,
                                           min_new_tokens=a.tokens)
            one()
            eng.stage_times(reset=True)
            eng.sync()
            t0 = time.perf_counter()
            for _ in range(2):
                res = one()
            eng.sync()
            dt = (time.perf_counter() - t0) / 2
            st = eng.stage_times()
            words = same = w_ok = w_tot = n_ref = 0
            differing = []
            for k in range(B3):
                n = len(res["token_timestamps"][k])
                text, ws = collate.decode_asr(vocab, [{"tokens": res["sequences"][k][:n], "token_timestamps": res["token_timestamps"][k],
                                                       "stride": (30.0, 0.0, 0.0)}])
                words += len(ws)
                if k in gold:
                    n_ref += 1
                    t_ok, ok_w, tot_w = words_match(text, ws, gold[k])
                    same += int(t_ok); w_ok += ok_w; w_tot += tot_w
                    if not t_ok:
                        differing.append(k)
            enc_ms, enc_calls = st["encoder"]
            enc_tf = 2.274e12 * B3 / (enc_ms / enc_calls) / 1e9 if enc_calls else None
            peak = 5000.0 if mode == "fp8_all" else 2500.0     # the subset mode keeps most encoder flops in bf16
            out["modes"][mode] = {"ms_per_step": dt * 1e3, "rtf": dt / (30.0 * B3), "aligned_words_per_s": words / dt,
                                  "stage_ms_per_step": {k_: round(val[0] / 2, 3) for k_, val in st.items()},
                                  "encoder_TFps": enc_tf, "encoder_frac_of_peak": (enc_tf / peak if enc_tf else None), "encoder_peak_TFps": peak,
                                  "golden_clips_identical_text": [same, n_ref], "golden_words_within_20ms": [w_ok, w_tot],
                                  "golden_clips_differing": differing,
                                  "parity_ok": (bool(same == n_ref and w_ok >= 0.99 * max(w_tot, 1)) if n_ref > 0 else None),
                                  "encoder_gemm": {"bf16": a.dtype, "fp8": f"{a.dtype}, fc1 in e4m3", "fp8_all": "e4m3 (q/k/v, fc1, fc2, cross-K/V projection)"}[mode],
                                  "cross_kv_cache": "e4m3" if mode != "bf16" else a.dtype}
        finally:
            eng.close()
    return out


def longform_parity(out, gold):
    """The merged long-form output against the reference's (tests/golden/e2e_bench_longform_golden.json: the same recording through
    transformers.pipeline(chunk_length_s=30) on the CPU in fp32, 29 seams merged by tokenizer._decode_asr, REF/transcribe.py:21-33):
    longest common word subsequence (a divergent chunk cannot shift everything behind it), words of it within 20 ms, identical text."""
    import difflib
    ref = gold["chunks"]
    sm = difflib.SequenceMatcher(a=[w["text"] for w in ref], b=[w["text"] for w in out["chunks"]], autojunk=False)
    matched = close = 0
    for blk in sm.get_matching_blocks():
        for k in range(blk.size):
            matched += 1
            ra, ob = ref[blk.a + k], out["chunks"][blk.b + k]
            close += int(all(abs(p_ - q_) <= 0.02 + 1e-9 for p_, q_ in zip(ra["timestamp"], ob["timestamp"])))
    return {"words": len(out["chunks"]), "reference_words": len(ref), "words_in_common_order": matched, "words_within_20ms": close,
            "identical_text": bool(out["text"] == gold["text"]),
            "word_for_word": bool(out["text"] == gold["text"] and close == len(ref) == len(out["chunks"])),
            "ok": bool(close >= 0.985 * len(ref))}


def longform_leg(a, dev, g, v, spec, vocab, shard, world, fence, max_over_ranks):
    """BASELINE configs[2]: one 600 s recording -> 30 chunks (30 s windows, 5 s strides) through the public pipeline call, chunk-sharded
    over the ranks (contiguous blocks, dist.shard_bounds), one all-gather of the per-chunk records, seam merge + pause split on every
    rank; everything from the host PCM array to the final word list is inside the timed call (PCIe included).  The headline number of
    the leg is taken at the REFERENCE's batch size (REF/transcribe.py:27: batch_size=16), with batch 8 and all-chunks-in-one-batch
    beside it, in the bench dtype AND in the other 16-bit dtype (f16 is the reference's own GPU dtype, REF/transcribe.py:10), and
    every merged output (before the pause split, which the reference record does not contain) is compared with the committed
    transformers output of the same recording."""
    import crisperwhisper_amd as cw
    from crisperwhisper_amd import audio as cw_audio, dist, synthetic as syn
    from crisperwhisper_amd.engine import Engine
    xl = syn.synth_audio(1000, a.longform_seconds * 16000, "mixed")
    gk = {"num_beams": 1, "language": "<|en|>", "task": "transcribe", "max_new_tokens": a.tokens, "min_new_tokens": a.tokens}
    n_chunks = len(cw_audio.chunk_windows(len(xl), 480000, 80000, 80000))
    shards = [h - l for l, h in dist.shard_bounds(n_chunks, world)]
    gold = None
    gpath = os.path.join(ROOT, "tests", "golden", "e2e_bench_longform_golden.json")
    if os.path.exists(gpath):
        gd = json.load(open(gpath))
        if (gd["audio"] == {"seed": 1000, "kind": "mixed", "secs": a.longform_seconds} and gd.get("weights") == a.weights and gd.get("weight_seed", 0) == 0
                and gd["generate_kwargs"]["max_new_tokens"] == a.tokens and gd["generate_kwargs"].get("min_new_tokens") == a.tokens):
            gold = gd
    mb = min(64, max(16, shards[0]))                  # decoder rows of the leg's engines: the reference batch size or one batch for all local chunks
    dtypes = [a.dtype] + [d for d in ("bf16", "f16") if d != a.dtype and a.dtype in ("bf16", "f16")]
    batches = sorted({min(8, mb), min(16, mb), min(mb, shards[0])})
    ref_batch = min(16, mb)
    out = None
    per_dtype = {}
    for dt_name in dtypes:
        eng = Engine(spec, dtype=dt_name, max_batch=mb, device=dev, cross_kv_dtype=None if a.cross_kv == "bf16" else a.cross_kv)
        try:
            for name, shape in syn.weight_shapes(g).items():
                eng.load_tensor(name, syn.weight_tensor(g, name, shape, 0, a.weights))
            rows = {}
            for bs in (batches if dt_name == a.dtype else [ref_batch]):
                pipe = cw.pipeline("automatic-speech-recognition", model=cw.ModelBundle(spec, {}), tokenizer=vocab, chunk_length_s=30,
                                   batch_size=bs, return_timestamps="word", device=f"cuda:{dev}", shard=shard, engines=[eng])
                pipe(xl, generate_kwargs=gk)                       # warm-up of this call path at this batch size (decode graphs of its row counts)
                fence()
                t0 = time.perf_counter()
                raw = pipe(xl, generate_kwargs=gk)
                t_p = time.perf_counter()
                res = cw.adjust_pauses_for_hf_pipeline_output({"text": raw["text"], "chunks": [dict(c) for c in raw["chunks"]]}, engine=eng)
                t_q = time.perf_counter()
                fence()
                lw = max_over_ranks(time.perf_counter() - t0)
                ph = dict(pipe.stats.get("last_call_phase_s", {}))
                ph["pause_split"] = t_q - t_p
                rows[bs] = {"wall_s": lw, "rtf": lw / a.longform_seconds, "aligned_words_per_s": len(res["chunks"]) / lw, "words": len(res["chunks"]),
                            # digest of the merged output (text + every word with its timestamps): the same at every rank count
                            "output_sha1": hashlib.sha1(json.dumps([res["text"], [[c["text"], list(c["timestamp"])] for c in res["chunks"]]]).encode()).hexdigest(),
                            "parity": longform_parity(raw, gold) if gold is not None else None,
                            # rank 0's wall time by phase: only `local_batches` shrinks with the rank count
                            "phase_s_rank0": {k: (round(v_, 4) if isinstance(v_, float) else v_) for k, v_ in ph.items()}}
            per_dtype[dt_name] = rows
        finally:
            eng.close()
    head = per_dtype[a.dtype][ref_batch]
    out = {"workload": f"BASELINE configs[2]: {a.longform_seconds} s recording -> {n_chunks} chunks (30 s, 5 s strides), "
                       f"contiguous chunk shards over {world} rank(s) = {shards}, batch_size {ref_batch} (REF/transcribe.py:27), {a.tokens} tokens/pass, "
                       f"one all-gather of {dist.REC_WORDS * 4}-byte chunk records, seam merge + pause split; untimed warm-up call of the same recording first",
           "batch_size": ref_batch, "dtype": a.dtype, "chunk_shards": shards, "scaling": "strong", "n_gpus": world}
    out.update(head)
    out["by_batch_size"] = {str(bs): {k: r[k] for k in ("wall_s", "rtf", "aligned_words_per_s", "words", "output_sha1")} | {"parity": r["parity"]}
                            for bs, r in per_dtype[a.dtype].items()}
    # configs[2] parity per dtype at the reference batch size, against the transformers output of the same recording
    out["parity"] = {d: dict(per_dtype[d][ref_batch]["parity"] or {}, wall_s=per_dtype[d][ref_batch]["wall_s"]) for d in per_dtype} if gold is not None else None
    out["parity_against"] = ("tests/golden/e2e_bench_longform_golden.json (transformers 5.15.0 pipeline, CPU fp32, chunk_length_s=30, batch_size=4, same recording / "
                             "aligned synthetic weights / token count; merged text + words before the pause split); ok = >= 98.5 % of the reference words "
                             "in common order and within 20 ms; word_for_word = identical text and every word within 20 ms") if gold is not None else None
    return out



def spawn_command(a, argv, port):
    """`python bench.py --gpus N` without a launcher: the command that re-runs this script as N ranks, one per GPU of this node
    (torch.distributed.run, rendezvous on 127.0.0.1 -- the container hostname may not resolve)."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
            "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)


def main():
    a = parse()
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # not under a launcher: spawn the ranks ourselves and relay rank 0's JSON line
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        rc = subprocess.call(spawn_command(a, sys.argv[1:], port), env=env)
        sys.exit(rc)
    # stdout carries exactly ONE line (the JSON record): everything else any library writes to fd 1 -- RCCL prints a five-line
    # version banner there, through C stdio, at communicator creation or at exit -- is diverted to stderr
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus and rank == 0:
        print(f"bench.py: --gpus {a.gpus} but the launcher started {world} rank(s); reporting n_gpus = {world}", file=sys.stderr)
    import torch  # imported before the native library so that one HIP runtime serves both
    import torch.distributed as td
    backend = os.environ.get("CW_DIST_BACKEND", "nccl")       # "gloo": lets 2 ranks share one GPU in a smoke test
    ndev = max(torch.cuda.device_count(), 1)
    if backend == "nccl" and world > ndev:
        # one process per GPU over RCCL: more ranks than devices would silently put two ranks on one GPU and report a curve that is
        # not a scaling curve (RCCL itself refuses duplicate devices later, with a less readable message).  CW_DIST_BACKEND=gloo is
        # the explicit opt-in for ranks sharing a device (tests/test_dist_gloo.py); the line then carries collective.emulated = true.
        if rank == 0:
            sys.stderr.write(f"bench.py: --gpus {world} over RCCL needs {world} visible devices, this node shows {ndev}; refusing "
                             "(CW_DIST_BACKEND=gloo runs the ranks on shared devices as an emulation)\n")
        sys.exit(4)
    dev = local % ndev
    pg = None            # "nccl" (= RCCL) / "gloo" / None
    pg_note = None
    if world > 1:
        torch.cuda.set_device(dev)
        if backend == "nccl":
            td.init_process_group("nccl", device_id=torch.device(f"cuda:{dev}"))
        else:
            td.init_process_group(backend)
        pg = backend
    elif backend == "nccl" and not a.no_rccl and torch.cuda.is_available():
        # single GPU: still bring up a one-rank RCCL communicator so the gather of the word records goes through
        # ncclAllGather on the 1-GPU lease too (the data path is identical at N = 1 and N = 8; only the peer count differs)
        try:
            torch.cuda.set_device(dev)
            if "RANK" in os.environ and "MASTER_ADDR" in os.environ:
                td.init_process_group("nccl", device_id=torch.device(f"cuda:{dev}"))
            else:
                import socket
                with socket.socket() as sk:
                    sk.bind(("127.0.0.1", 0))
                    port = sk.getsockname()[1]
                td.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                                      device_id=torch.device(f"cuda:{dev}"))
            pg = "nccl"
        except Exception as e:       # never take the bench down with it: report and run without a communicator
            pg_note = f"RCCL communicator not available at world=1: {e!r}"
    from crisperwhisper_amd import collate, dist, generation, synthetic as syn, utils
    from crisperwhisper_amd.engine import Engine

    g, v = syn.large_v3_geometry() if a.geometry == "large-v3" else syn.tiny_geometry()
    spec = syn.model_spec(g, v, n_align=15 if a.geometry == "large-v3" else 3)
    B = a.batch
    C = max(1, a.contexts)
    engines = [Engine(spec, dtype=a.dtype, max_batch=B * max(1, a.num_beams), device=dev, cross_kv_dtype=None if a.cross_kv == "bf16" else a.cross_kv)
               for _ in range(C)]
    eng = engines[0]
    keep = a.full and (not a.no_cpu_baseline) and world == 1 and rank == 0
    keep_weights = keep and a.cpu_port
    weights = {}
    t0 = time.perf_counter()
    for name, shape in syn.weight_shapes(g).items():
        w = syn.weight_tensor(g, name, shape, 0, a.weights)
        for e_ in engines:
            e_.load_tensor(name, w)
        if keep_weights:
            weights[name] = w
    t_load = time.perf_counter() - t0
    if a.encoder_gemm == "fp8":
        for e_ in engines:
            e_.check_weights()
            e_.set_encoder_gemm_fp8(True)
    vocab = collate.Vocabulary.from_synthetic(v)
    utils.bind_engine(eng)
    shard = dist.Shard(rank, world, device=f"cuda:{dev}" if pg == "nccl" else None, collective_at_world1=(pg is not None))

    nfs = []
    for ci, e_ in enumerate(engines):
        clips = [syn.synth_audio((rank * C + ci) * B + i, 480000, "noise") for i in range(B)]
        nfs.append(e_.upload_pcm(clips))             # inputs resident in HBM before the timed region
    audio_s = 30.0 * B * C

    last_raw = {}                                     # rank-local words of the latest step (before the pause split)
    last_out = {}                                     # the latest step's generate() result per context, and the gathered records

    def step_ctx(ci):
        eng, nf = engines[ci], nfs[ci]
        eng.mel_resident(B)
        out = generation.generate(eng, B, nf, language="<|en|>", task="transcribe", max_new_tokens=a.tokens,
                                  min_new_tokens=a.tokens, num_beams=a.num_beams)
        last_out[ci] = out
        # every chunk is an independent clip here, so each rank collates + pause-splits its own chunks and the
        # ranks exchange the per-chunk *word lists* (one small all-gather); rank 0 ends up with all results
        recs = []
        n_tokens = 0
        for k in range(B):
            n = len(out["token_timestamps"][k])
            n_tokens += n
            text, words = collate.decode_asr(vocab, [{"tokens": out["sequences"][k][:n],
                                                      "token_timestamps": out["token_timestamps"][k],
                                                      "stride": (30.0, 0.0, 0.0)}])
            if ci == 0:
                last_raw[k] = {"text": text, "chunks": [{"text": w_["text"], "timestamp": tuple(w_["timestamp"])} for w_ in words]}
            res = utils.adjust_pauses_for_hf_pipeline_output({"text": text, "chunks": words}, engine=eng)
            recs.append(dist.pack_words((rank * C + ci) * B + k, res["chunks"]))
        return recs, n_tokens

    def step():
        if C == 1:
            parts = [step_ctx(0)]
        else:
            import concurrent.futures as cf
            with cf.ThreadPoolExecutor(C) as ex:
                parts = list(ex.map(step_ctx, range(C)))
        recs = [r for p_ in parts for r in p_[0]]
        n_tokens = sum(p_[1] for p_ in parts)
        allr = shard.all_gather_records(np.stack(recs), B * C)
        last_out["records"] = allr
        n_words = 0
        if rank == 0:
            for r in allr:
                _, words = dist.unpack_words(r)
                n_words += len(words)
        n_tokens *= world                             # every rank decodes the same number of tokens per chunk
        return n_words, n_tokens

    def fence():
        for e_ in engines:
            e_.sync()
        if pg is not None:
            td.barrier()
        torch.cuda.synchronize()

    for _ in range(a.warmup):
        step()
    for e_ in engines:
        e_.stage_times(reset=True)
    fence()
    t0 = time.perf_counter()
    words = tokens = 0
    for _ in range(a.steps):
        w, t = step()
        words += w
        tokens += t
    fence()
    dt = time.perf_counter() - t0
    if a.dump_outputs and rank == 0:
        local = {(rank * C + ci) * B + k: (last_out[ci]["sequences"][k], last_out[ci]["token_timestamps"][k])
                 for ci in range(C) for k in range(B)}
        dump_outputs(a.dump_outputs, last_out["records"], local, spec.pad_token_id)

    def max_over_ranks(x):
        if pg is None:
            return x
        tt = torch.tensor([x], dtype=torch.float64, device=f"cuda:{dev}" if pg == "nccl" else "cpu")
        td.all_reduce(tt, op=td.ReduceOp.MAX)
        return float(tt.item())

    dt_local = dt

    def over_ranks(x, op):
        if pg is None:
            return x
        tt = torch.tensor([x], dtype=torch.float64, device=f"cuda:{dev}" if pg == "nccl" else "cpu")
        td.all_reduce(tt, op=op)
        return float(tt.item())

    dt = max_over_ranks(dt)
    dt_min = over_ranks(dt_local, td.ReduceOp.MIN) if pg is not None else dt_local
    n_gathers = shard.n_collectives
    gather_us = shard.gather_s / max(n_gathers, 1) * 1e6          # this rank's average; the slowest rank's is reduced below
    gather_us_max = over_ranks(gather_us, td.ReduceOp.MAX) if pg is not None else gather_us
    stages = eng.stage_times()
    for e_ in engines[1:]:
        for k_, (ms_, n_) in e_.stage_times().items():
            stages[k_] = (stages[k_][0] + ms_, stages[k_][1] + n_)

    # ---- the timed output against the reference: the clips of rank 0 are the ones tests/golden/gen_golden_bench.py ran
    # through transformers (CPU, fp32) with the same aligned weights and token count
    parity = None
    if a.full and rank == 0 and a.geometry == "large-v3" and a.dtype in ("bf16", "f16"):
        gold = load_bench_goldens(a.tokens, a.weights) if a.num_beams == 1 else load_beam_goldens(a.tokens, a.weights, a.num_beams)
        ks = [k for k in range(B) if k in gold and k in last_raw]
        if ks:
            same_text = w_ok = w_tot = 0
            for k in ks:
                t_ok, ok_w, tot_w = words_match(last_raw[k]["text"], last_raw[k]["chunks"], gold[k])
                same_text += int(t_ok); w_ok += ok_w; w_tot += tot_w
            # BASELINE configs[5] harness (timestamp F1 / IoU at a 0.2 s collar vs the reference) on the same pairs
            from crisperwhisper_amd import metrics
            f1s = [metrics.boundary_f1(gold[k]["chunks"], last_raw[k]["chunks"], 0.2)[2] for k in ks]
            ious = [metrics.mean_iou(gold[k]["chunks"], last_raw[k]["chunks"]) for k in ks]
            parity = {"timestamp_f1_collar_0.2s": float(np.mean(f1s)), "mean_word_iou": float(np.mean(ious)),
                      "against": ("tests/golden/e2e_bench_golden.json + e2e_bench_b64_golden.json" if a.num_beams == 1 else "tests/golden/e2e_bench_beam128_golden.json")
                                 + " (transformers 5.15.0 pipeline, CPU fp32, same clips / weights / token count)",
                      "mode": ("free-running greedy" if a.num_beams == 1 else f"free-running beam search x{a.num_beams}") + ", the timed path itself", "clips_with_identical_text": [same_text, len(ks)],
                      # how much this block can carry (crisperwhisper_amd/synthetic.py:244-301): no trained checkpoint exists offline, so the
                      # weights are seeded synthetic tensors whose alignment heads are peaked by construction -- the DTW ridge is set by the
                      # decoder POSITION (token t at frame 11 t, ~3 sigma above the content terms), so the timestamp half of this check is
                      # weakly sensitive to encoder / cross-attention error; the text half (argmax over 51866 logits, free-running) is not.
                      # The i.i.d.-weight f32 tests and the bit-exact DTW / median kernel tests carry the fine-grained weight.
                      "caveat": "aligned SYNTHETIC weights: timestamps are position-determined by construction (weakly sensitive to encoder / cross-attention error); text parity is free-running argmax; no trained checkpoint offline",
                      "words_identical_and_within_20ms": [w_ok, w_tot],
                      "ok": bool(same_text == len(ks) and w_tot > 0 and w_ok >= 0.99 * w_tot)}

    # ---- BASELINE configs[2]: one long recording -> 30 s chunks with 5 s strides, chunk-sharded over the ranks
    # (contiguous blocks, dist.shard_bounds), one all-gather of the per-chunk records, seam merge + pause split on every
    # rank.  Everything from the host PCM array to the final word list is inside the timed call (PCIe included).
    longform = None
    if a.full and a.geometry == "large-v3" and not a.no_longform and C == 1 and a.num_beams == 1:
        longform = longform_leg(a, dev, g, v, spec, vocab, shard, world, fence, max_over_ranks)
    # roofline of the decode step: EVERY launch of the decoder layer as the step issues it at this batch (cw_time_decode_stage runs
    # the step's own launch code one stage at a time) + the logits projection, HIP events on the engine's own stream
    roof = []
    if a.full and a.num_beams == 1:
        for st in eng.time_decode_stages(B, a.kernel_iters):
            roof.append({"kernel": st["kernel"], "stage": st["stage"], "avg_ms": st["avg_ms"], "algo_bytes": st["algo_bytes"], "per_step": g.dec_layers,
                         "launches": st.get("launches", 1)})
        ms, by = eng.time_kernel(7, B, a.kernel_iters)
        roof.append({"kernel": "LayerNorm + logits projection (gemv_loop_kernel)", "stage": 100, "avg_ms": ms, "algo_bytes": by, "per_step": 1})
    elif a.full:   # beam rows: the two kernels of the greedy layer that dominate it (the beam layer's own launches are in the rocprofv3 table)
        for which, kname in ((0, "LayerNorm + fc1 + GELU"), (1, "cross-attention")):
            ms, by = eng.time_kernel(which, B, a.kernel_iters)
            roof.append({"kernel": kname, "stage": which, "avg_ms": ms, "algo_bytes": by, "per_step": g.dec_layers})
    for r_ in roof:
        r_["achieved"] = r_["algo_bytes"] / (r_["avg_ms"] * 1e-3) / 1e9 if r_["avg_ms"] > 0 else 0.0

    def pmc_traffic(kernel_substr):
        """HBM bytes per launch of the kernel from the committed rocprofv3 PMC pass (profiles/, same batch)."""
        try:
            t = json.load(open(os.path.join(ROOT, "profiles", PMC_FILE)))
            if t.get("batch") != B:
                return None
            for k, val in t["kernels"].items():
                if kernel_substr in k:
                    return val["hbm_read_bytes_per_launch"]
        except Exception:
            pass
        return None

    if rank == 0:
        total_audio = audio_s * world * a.steps
        # dominant kernel = the launch with the largest MEASURED share of the decode step (avg launch time x launches per step)
        singles = [r_ for r_ in roof if r_["stage"] >= 0]
        dec_ms, dec_calls = stages["decode"]
        dec_step_ms = (dec_ms / dec_calls / (1 if a.num_beams > 1 else a.tokens + 2)) if dec_calls else None
        for r_ in roof:
            r_["share_of_decode_step"] = (r_["avg_ms"] * r_["per_step"] / dec_step_ms) if dec_step_ms else None
        r = max(singles, key=lambda r_: r_["avg_ms"] * r_["per_step"]) if singles else None     # None: no roofline runs (no --full)
        PMC_NAMES = {"cross-attention": "attn_cross_mfma8" if a.cross_kv == "fp8" else "attn_cross_split_kernel", "qkv_self_kernel": "qkv_self_kernel",
                     "gemv_stack_kernel": "gemv_stack_kernel", "fc1": "gemv2_bf16_kernelILi1E", "fc2": "gemv2_bf16_kernelILi2ELi2ELb1ELb0",
                     "out-projection (combines": "gemv2_bf16_kernelILi2ELi1ELb1ELb1", "logits": "gemv_loop_kernel"}

        def pmc_of(kernel_label):
            for key, sub in PMC_NAMES.items():
                if key in kernel_label and not (key == "cross-attention" and "out-projection" in kernel_label):
                    return pmc_traffic(sub)
            return None
        line = {
            "metric": "aligned words/s (RTF alongside), CrisperWhisper large-v3 geometry, 30 s chunks, full mel->encoder->decoder->DTW->words path",
            "value": words / dt, "unit": "aligned words/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": dt / a.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": a.dtype, "data": "synthetic",
            "rtf": dt / total_audio, "tokens_per_s": tokens / dt,
            "config": {"workload": f"BASELINE configs[1]: batch={B} x 30 s synthetic 16 kHz audio per GPU, {a.dtype}, "
                                   f"{a.tokens} generated tokens/chunk, geometry {a.geometry}, {a.weights} synthetic weights, "
                                   + ("greedy" if a.num_beams == 1 else f"beam search x{a.num_beams} [not the BASELINE configuration]") + ", word timestamps"
                                   + (", fp8 (e4m3) cross-attention cache [opt-in mode]" if a.cross_kv == "fp8" else "")
                                   + (", fp8 (e4m3) encoder / cross-K/V GEMMs [opt-in mode]" if a.encoder_gemm == "fp8" else ""),
                       "chunks_per_gpu": B * C, "contexts_per_gpu": C, "tokens_per_chunk": a.tokens, "parallelism": f"chunk-dp{world}",
                       "cross_kv_cache": a.cross_kv, "encoder_gemm": a.encoder_gemm, "num_beams": a.num_beams, "weight_load_s": round(t_load, 1)},
            "stage_ms_per_step": {k: round(val[0] / max(a.steps, 1) / C, 3) for k, val in stages.items()},
            "roofline": {"bound": "hbm", "achieved": r["achieved"], "peak": 8000.0, "unit": "GB/s",
                         "frac": r["achieved"] / 8000.0,
                         "traffic": pmc_of(r["kernel"]),
                         "traffic_source": f"profiles/{PMC_FILE}: separate rocprofv3 --pmc FETCH_SIZE pass of this command at the same batch and --tokens 32 (x2 gfx950 correction; with a TCC counter rocprofv3 segfaults at --tokens 128, and the per-launch traffic does not depend on the token count), not re-measured in this run",
                         "kernel": r["kernel"],
                         "avg_launch_ms": r["avg_ms"], "algorithmic_bytes_per_launch": r["algo_bytes"],
                         "launches_per_decode_step": r["per_step"], "share_of_decode_step": r["share_of_decode_step"],
                         "dominant_by": "largest measured share of the decode step among all launches of the layer + logits (roofline_other lists the rest)",
                         # the step as a whole (filled in below from the stage timers): algorithmic bytes of one token step / its time
                         "step_frac": None, "step_achieved": None} if r is not None else None,
            "parity": parity,
            "collective": {"backend": ("rccl (torch.distributed nccl)" if pg == "nccl" else pg), "all_gathers_in_timed_region": n_gathers,
                           # true = not a hardware scaling measurement: the ranks meet over gloo (host TCP) and may share devices
                           "emulated": bool(pg == "gloo"), "ranks_per_device": (world + ndev - 1) // ndev,
                           "ranks_seen": (td.get_world_size() if pg is not None else 1), "devices_visible": ndev,
                           "chunks_per_rank": [B * C] * world, "note": pg_note,
                           # > 0 only when this rank's GPU is shared with other work: calls repeated on the launch-per-stage decoder kernels
                           "handoff_fallbacks_rank0": sum(int(e_.lib.cw_handoff_fallbacks(e_.ctx)) for e_ in engines),
                           # what a reader needs to hold an N-GPU line against the N = 1 line: every rank runs the
                           # N = 1 workload, so per-rank ms_per_step must equal the N = 1 ms_per_step and value must be N x the N = 1 value
                           "per_rank_ms_per_step": {"min": dt_min / a.steps * 1e3, "max": dt / a.steps * 1e3},
                           "gather_us_per_call": {"rank0": gather_us, "max_over_ranks": gather_us_max},
                           "gather_bytes_per_rank": int(B * C * dist.WORD_REC * 4) if hasattr(dist, "WORD_REC") else None,
                           "expect": "weak scaling: value(N) = N x value(1) x (1 - gather / step), per-rank ms_per_step = N = 1 ms_per_step; DESIGN.md section 5 holds the prediction"},
            "longform": longform,
            "roofline_other": [{"kernel": r_["kernel"], "achieved_GBps": r_["achieved"], "frac_of_8TBps": r_["achieved"] / 8000.0,
                                "avg_launch_ms": r_["avg_ms"], "algorithmic_bytes_per_launch": r_["algo_bytes"],
                                "launches_per_decode_step": r_["per_step"], "share_of_decode_step": r_["share_of_decode_step"],
                                "traffic": pmc_of(r_["kernel"])}
                               for r_ in roof if r_ is not r] if r is not None else None,
        }
        # per-stage achieved fraction of roofline (BASELINE.md section 3 work figures; times = HIP events per call)
        if a.geometry == "large-v3":
            def per_call(stage):
                ms, calls = stages[stage]
                return (ms / calls) if calls else None
            sr = {}
            t = per_call("mel")
            if t:
                by = 3456000.0 * B
                sr["mel"] = {"bound": "hbm", "algorithmic_bytes": by, "ms_per_call": t, "achieved_GBps": by / t / 1e6,
                             "frac_of_8TBps": by / t / 1e6 / 8000.0, "note": "folded 400-point DFT on the f64 matrix cores (v_mfma_f64_16x16x4_f64: issue-bound, ~29 TFLOP/s f64 measured); an f32 product would sit 7-9e-5 from the reference on pure tones (bar 1e-4)"}
            t = per_call("encoder")
            if t:
                fl = 2.274e12 * B
                sr["encoder"] = {"bound": "mfma", "algorithmic_flops": fl, "ms_per_call": t, "achieved_TFps": fl / t / 1e9,
                                 "frac_of_2500TFps": fl / t / 1e9 / 2500.0}
            t = per_call("cross_kv")
            if t:
                fl = 3.146e11 * B
                sr["cross_kv"] = {"bound": "mfma", "algorithmic_flops": fl, "ms_per_call": t, "achieved_TFps": fl / t / 1e9,
                                  "frac_of_2500TFps": fl / t / 1e9 / 2500.0}
            ms, calls = stages["decode"]
            if calls:
                steps_per_call = a.tokens + 2            # prompt positions 0,1 + one forward per generated token
                by = 1.812e9 + B * 245.76e6 * (0.5 if a.cross_kv == "fp8" else 1.0)   # weights (bf16) + cross-K/V per step (e4m3 cache: one byte per element); self-K/V omitted
                per_step_ms = ms / calls / steps_per_call
                if a.num_beams > 1:                       # beam search: the stage timer brackets every cw_beam_step (one forward of B x beams rows)
                    per_step_ms = ms / calls
                # streamed = what the kernels actually read: the fused out-projection / cross-query stage (csrc/decfuse.hip) adds a
                # d x d product matrix per layer to the weight stream; the fraction is quoted on the ALGORITHMIC bytes
                # (rows <= 16, and 17..64 rows over either cache: there the stage runs in groups of 16 rows; CW_NO_FUSE_ROWS=1 / CW_NO_FUSE_ROWS8=1 switch it off)
                # (engine.hip decode_step: `fuse`)
                fused_stage = (a.dtype in ("bf16", "f16") and a.num_beams == 1 and not os.environ.get("CW_NO_FUSE6") and
                               (B <= 16 or (B <= 64 and not os.environ.get("CW_NO_FUSE_ROWS") and
                                            (a.cross_kv != "fp8" or not os.environ.get("CW_NO_FUSE_ROWS8")))))
                streamed = by + (g.dec_layers * g.d_model * g.d_model * 2.0 if fused_stage else 0.0)
                sr["decode_step"] = {"bound": "hbm", "algorithmic_bytes": by, "streamed_bytes": streamed, "ms_per_step": per_step_ms,
                                     "achieved_GBps": by / per_step_ms / 1e6, "frac_of_8TBps": by / per_step_ms / 1e6 / 8000.0,
                                     # kernel launches (a 17..64-row LayerNorm / combining GEMV is a preparation launch + the GEMV: counted as two)
                                     # (greedy: counted by the roofline runs of --full, None without them)
                                     "launches_per_layer": ((sum(r_.get("launches", 1) for r_ in roof if 0 <= r_["stage"] < 100) if roof else None)
                                                            if a.num_beams == 1 else (12 if B * a.num_beams > 16 else 8))}
                if a.num_beams > 1:
                    sr["decode_step"]["rows"] = B * a.num_beams
                if line["roofline"] is not None:
                    line["roofline"]["step_frac"] = sr["decode_step"]["frac_of_8TBps"]
                    line["roofline"]["step_achieved"] = sr["decode_step"]["achieved_GBps"]
                    line["roofline"]["sum_of_launch_shares"] = sum(r_["share_of_decode_step"] for r_ in roof if r_["stage"] >= 0 and r_["share_of_decode_step"] is not None)
            t = per_call("timestamps")
            if t:
                by = 4.0 * 15 * a.tokens * 1500 * B
                sr["token_timestamps"] = {"bound": "hbm (pre-pass) / dependency chain (DTW)", "algorithmic_bytes": by,
                                          "ms_per_call": t, "achieved_GBps": by / t / 1e6,
                                          "dtw_us_per_antidiagonal": t * 1e3 / (a.tokens + 1500 - 1)}
            line["stage_roofline"] = sr
            line["passes_per_step"] = stages["encoder"][1] / max(a.steps, 1)
        if a.full and a.geometry == "large-v3" and world == 1 and not a.no_config3 and a.dtype in ("bf16", "f16") and a.num_beams == 1:
            for e_ in engines:
                e_.close()
            engines = []
            try:
                line["config3"] = config3_leg(a, dev, g, v, spec)
            except Exception as e:                   # never take the headline down with it
                line["config3"] = {"error": repr(e)}
        if keep:
            for e_ in engines:                       # free the GPU side first: the CPU legs need the host memory bandwidth
                e_.close()
            engines = []
            try:
                line["cpu_baseline"] = cpu_reference(a.geometry, a.tokens, a.cpu_threads, a.cpu_timeout, a.weights)
            except Exception as e:  # the baseline leg must never take the GPU number down with it
                line["cpu_baseline"] = {"value": None, "unit": "aligned words/s", "cores": os.cpu_count(), "kind": "reference",
                                        "sample": f"failed: {e!r}"}
            if a.cpu_port:
                try:
                    line["cpu_baseline"]["port"] = cpu_baseline(g, v, spec, weights, a.tokens, words / max(a.steps * B * C * world, 1), a.cpu_tokens)
                except Exception as e:
                    line["cpu_baseline"]["port"] = {"value": None, "kind": "port", "sample": f"failed: {e!r}"}
        os.write(json_fd, (json.dumps(line) + "\n").encode())
    for e_ in engines:
        e_.close()
    if pg is not None:
        td.destroy_process_group()
    # a fast result that differs from the reference's is not a result: the line is printed (the mismatch is in it), the exit
    # status says so.  The everything-e4m3 mode (fp8_all) of the configs[3] leg is accuracy-gated by its own tests and does not count here.
    if rank == 0:
        bad = []
        if parity is not None and not parity["ok"] and a.num_beams == 1:   # beam search: reported in the line, not part of the exit status
            bad.append("headline")
        for d_, p_ in ((longform or {}).get("parity") or {}).items():
            if p_ and p_.get("ok") is False:
                bad.append(f"longform {d_}")
        c3 = line.get("config3") or {}
        for m_ in ("bf16", "fp8"):
            if isinstance(c3.get("modes"), dict) and c3["modes"].get(m_) and c3["modes"][m_].get("parity_ok") is False:
                bad.append(f"config3 {m_}")
        if bad:
            sys.stderr.write("bench.py: PARITY FAILED (" + ", ".join(bad) + "): the output differs from the committed transformers reference\n")
            sys.exit(3)


if __name__ == "__main__":
    main()
