"""Forced alignment of known transcripts on the device (cw_align_tokens, Engine.align_tokens, CrisperWhisperPipeline.align).

* The prefill attention's alignment recording (prefill_attn_kernel, cross mode) against a float64 softmax, and its `out`
  bit-identical to the kernel without recording.
* At the bench geometry (large-v3, aligned synthetic weights, 8 x 30 s clips): the teacher-forced sequences transformers
  produced for tests/golden/e2e_bench_golden.json, aligned, against transformers' own token timestamps of those sequences and
  against what the engine's greedy decode of the same sequences leaves behind; the prefill against the per-position loop.
* Ragged batches: every row's timestamps bit-identical to the row aligned on its own, on every engine and both forward paths.
* The pipeline surface: aligning the ids a transcription generated reproduces its words; refusals of the C ABI.

Error bound of the kernel test (16-bit q, k rounded on upload; the reference is float64 over those rounded values).  The
kernel's score s = q . k is an f32 MFMA accumulation of 64 exact products (8- or 11-bit mantissas: the products fit f32), so
|s - s64| <= 64 u A with u = 2^-24 and A = sum_i |q_i k_i| (the classic bound for n-term recursive summation, n u A).  The
weight exp(s - m) / l then carries: 2 max|s - s64| from the score of the key and the maximum m (a shift cancels in the ratio
but the row's maximum comes from another key), the exponential's relative error (v_exp_f32 after the log2(e) scaling: 2^-21
plus |s - m| u for the rounded argument), the f32 sum l over n_keys terms (n_keys u relative) and the final normalise
multiply (2 u).  So |w - w64| <= w64 (2 E + 2^-21 + |s - m| u + n_keys u + 2 u) + 1e-12 with E = 64 u max_j A_j per row.
"""
import numpy as np
import pytest

import crisperwhisper_amd as cw
from crisperwhisper_amd import collate, generation, synthetic as syn
from crisperwhisper_amd.engine import Engine, EngineError
from tests import helpers as Hh

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _round16(x, dtype):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x, np.float32))
    return (t.to(torch.bfloat16) if dtype == "bf16" else t.to(torch.float16)).to(torch.float32).numpy()


@pytest.fixture(scope="module")
def tiny():
    return Hh.tiny_setup()


def _engine(spec, W, dtype, rows=8):
    e = Engine(spec, dtype=dtype, max_batch=rows)
    e.load_state_dict(W)
    return e


# ---------------------------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("n_q", [1, 15, 16, 17, 131])
def test_prefill_alignment_rows_vs_float64(tiny, dtype, n_q):
    g, v, W, spec = tiny
    eng = _engine(spec, W, dtype, rows=4)
    try:
        rng = np.random.default_rng(1000 + n_q)
        H, S = 3, 1500
        for kv_div in (1, 2):
            rows = 4
            q = rng.standard_normal((rows, n_q, H * 64)).astype(np.float32) * 0.35
            k = rng.standard_normal((rows // kv_div, H, S, 64)).astype(np.float32) * 0.35
            vv = rng.standard_normal((rows // kv_div, H, S, 64)).astype(np.float32)
            ah = 1
            # sharp peaks on keys 0, 31 / 32 and 1499 for some queries of the alignment head (score ~ 14)
            for i, key in zip(range(n_q), [0, 31, 32, 1499]):
                for r in range(0, rows, kv_div):                      # rows r .. r + kv_div - 1 share K / V
                    qv = q[r, i, ah * 64:(ah + 1) * 64]
                    k[r // kv_div, ah, key] = qv / max(np.dot(qv, qv), 1e-6) * 14.0
            q, k, vv = (_round16(t, dtype) for t in (q, k, vv))
            out, al = eng.test_prefill_align_attention(q, k, vv, kv_div=kv_div, align_head=ah)
            plain = eng.test_prefill_attention(q, k, vv, S, False, kv_div)
            assert np.array_equal(out.view(np.uint32), plain.view(np.uint32)), "recording changed the attention output"
            for r in range(rows):
                qh = q[r, :, ah * 64:(ah + 1) * 64].astype(np.float64)
                kh = k[r // kv_div, ah].astype(np.float64)
                s = qh @ kh.T                                                  # [n_q][S]
                m = s.max(axis=1, keepdims=True)
                w64 = np.exp(s - m)
                w64 /= w64.sum(axis=1, keepdims=True)
                A = np.abs(qh) @ np.abs(kh).T
                E = 64 * U * A.max(axis=1, keepdims=True)
                bound = w64 * (2 * E + 2.0 ** -21 + np.abs(s - m) * U + S * U + 2 * U) + 1e-12
                err = np.abs(al[r].astype(np.float64) - w64)
                assert np.all(err <= bound), (kv_div, r, float((err - bound).max()), np.unravel_index(np.argmax(err - bound), err.shape))
                if n_q >= 4 and r % kv_div == 0:
                    assert np.argmax(al[r, 0]) == 0 and np.argmax(al[r, 3]) == 1499
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------- bench geometry vs HF
def _aligned_weights(g, seed=0):
    class Lazy(dict):                               # stream the f32 tensors one at a time
        def items(self):
            for n, shape in syn.weight_shapes(g).items():
                yield n, syn.weight_tensor(g, n, shape, seed, "aligned")
    return Lazy()


def _bench(dtype):
    gold = Hh.gold_json("e2e_bench_golden.json")
    g, v = syn.large_v3_geometry()
    spec = syn.model_spec(g, v, n_align=15)
    eng = Engine(spec, dtype=dtype, max_batch=8)
    eng.load_state_dict(_aligned_weights(g, gold["weight_seed"]))
    _, nf = eng.mel([syn.synth_audio(c["seed"], int(c["secs"] * 16000), c["kind"]) for c in gold["clips"]])
    seqs = [np.asarray(c["passes"][0]["sequences"][0], np.int64) for c in gold["clips"]]
    ref = [np.asarray(c["passes"][0]["token_timestamps"][0], np.float64) for c in gold["clips"]]
    n_init = gold["clips"][0]["passes"][0]["num_input_ids"]
    return eng, nf, seqs, ref, n_init


def _greedy(eng, nf, n_init, init, T):
    """A free-running greedy generation of the 8 windows (bench.py's decode: T - n_init forced-length tokens, nothing forced)
    and the token timestamps it leaves behind."""
    eng.encode(list(range(8)), [0] * 8, [3000] * 8)
    seq, lens, _ = eng.decode(np.tile(np.asarray(init, np.int32), (8, 1)), max_length=T, min_new_tokens=T - n_init)
    assert lens.tolist() == [T] * 8
    return [seq[k, :T].astype(np.int64) for k in range(8)], eng.token_timestamps(8, T - 1, n_init, nf)


def test_bench_geometry_f32_alignment_vs_transformers_and_greedy_generation():
    """f32: the 8 teacher-forced sequences of the golden (3 init tokens + 128 generated), aligned in one call: every token
    timestamp within 20 ms of transformers'.  Then a free-running greedy generation of the same windows; its ids, aligned:
    token timestamps bit-identical to the ones the generation produced."""
    eng, nf, seqs, ref, n_init = _bench("f32")
    try:
        got = eng.align_tokens(nf, seqs, n_init)
        for k in range(8):
            assert len(got[k]) == len(seqs[k])
            assert np.abs(got[k] - ref[k]).max() <= 0.02 + 1e-6, k
        T = len(seqs[0])
        gen, gen_ts = _greedy(eng, nf, n_init, seqs[0][:n_init], T)
        again = eng.align_tokens(nf, gen, n_init)
        for k in range(8):
            assert np.array_equal(again[k], gen_ts[k]), k
        assert eng.align_prefill_runs() == 0                          # the f32 engine runs the per-position loop
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_bench_geometry_16bit_prefill_vs_transformers_and_loop(dtype):
    """16-bit engines: the prefill forward (csrc/prefill.hip; the engine counts the calls that ran it) against transformers'
    timestamps of the same sequences, against the per-position loop (align_prefill = 0), and -- aligning the ids of a free-running
    greedy generation -- against the timestamps that generation produced: >= 99 % of the tokens within 20 ms in all three."""
    eng, nf, seqs, ref, n_init = _bench(dtype)
    try:
        pf = eng.align_tokens(nf, seqs, n_init)
        assert eng.align_prefill_runs() == 1
        eng.set_align_prefill(False)
        loop = eng.align_tokens(nf, seqs, n_init)
        assert eng.align_prefill_runs() == 1
        eng.set_align_prefill(True)
        a, b, r = (np.concatenate(x) for x in (pf, loop, ref))
        near_ref = np.mean(np.abs(a - r) <= 0.02 + 1e-6)
        near_loop = np.mean(np.abs(a - b) <= 0.02 + 1e-6)
        assert near_ref >= 0.99, near_ref
        assert near_loop >= 0.99, near_loop
        gen, gen_ts = _greedy(eng, nf, n_init, seqs[0][:n_init], len(seqs[0]))
        again = np.concatenate(eng.align_tokens(nf, gen, n_init))
        assert eng.align_prefill_runs() == 2
        near_gen = np.mean(np.abs(again - np.concatenate(list(gen_ts))) <= 0.02 + 1e-6)
        assert near_gen >= 0.99, near_gen
    finally:
        eng.close()


# --------------------------------------------------------------------------------------------------- batch independence
@pytest.mark.parametrize("dtype,prefill", [("f32", True), ("bf16", True), ("f16", True), ("bf16", False)])
def test_ragged_batch_rows_are_independent(tiny, dtype, prefill):
    """Rows of 5 .. 140 ids over clips of different lengths (num_frames 3000 down to 300), aligned as one batch and one row
    per call: bit-identical timestamps for every row."""
    g, v, W, spec = tiny
    eng = _engine(spec, W, dtype, rows=6)
    try:
        eng.set_align_prefill(prefill)
        rng = np.random.default_rng(7)
        secs = [30.0, 12.5, 3.0, 30.0, 7.0, 29.0]
        clips = [syn.synth_audio(300 + i, int(s * 16000), "mixed") for i, s in enumerate(secs)]
        lengths = [140, 5, 37, 37, 6, 64]                 # rows 2, 3: one length, different audio (one timestamp pass)
        init = [v.sot, v.lang_id("en"), v.transcribe]
        seqs = [np.concatenate([init, rng.integers(0, 256, n - 4), [v.eos]]).astype(np.int64) for n in lengths]
        _, nf = eng.mel(clips)
        assert len(set(nf.tolist())) > 2
        batch = eng.align_tokens(nf, seqs, 3)
        assert eng.align_prefill_runs() == (1 if prefill and dtype != "f32" else 0)
        for k in range(len(seqs)):
            _, nf1 = eng.mel([clips[k]])
            one = eng.align_tokens(nf1, [seqs[k]], 3)[0]
            assert np.array_equal(one, batch[k]), (k, lengths[k])
            assert len(one) == lengths[k] and np.all(one[:3] == 0) and one[-1] == one[-2]
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------- pipeline
def test_pipeline_align_reproduces_its_own_decode(tiny):
    """f32: the ids one greedy decode of a clip generated (text and timestamp tokens), aligned through
    CrisperWhisperPipeline.align, give exactly the words collate.decode_asr makes of that decode's own tokens and token
    timestamps; a list of inputs gives one dict per input; the output goes through adjust_pauses_for_hf_pipeline_output;
    language=None detects the language per item."""
    g, v, W, spec = tiny
    vocab = collate.Vocabulary.from_synthetic(v)
    pipe = cw.pipeline("automatic-speech-recognition", model=cw.ModelBundle(spec, W), tokenizer=vocab,
                       batch_size=2, return_timestamps="word", torch_dtype="float32", device="cuda:0")
    try:
        clips = [syn.synth_audio(11, 20 * 16000, "mixed"), syn.synth_audio(12, 9 * 16000, "mixed")]
        eng = pipe.engine
        init = np.array([[v.sot, v.lang_id("en"), v.transcribe]], np.int32)
        texts, want = [], []
        for c in clips:
            _, nf = eng.mel([c])
            eng.encode([0], [0], [3000])
            seq, lens, _ = eng.decode(init, max_length=60)
            n = int(lens[0])
            ts = eng.token_timestamps(1, n - 1, 3, nf)[0]
            text = seq[0, 3:n - 1].astype(np.int64)          # the last id is only predicted (eos, or the length cap)
            texts.append(text)
            want.append(collate.decode_asr(vocab, [{"tokens": text, "token_timestamps": ts[3:3 + len(text)]}]))
        got = pipe.align(clips, texts, language="<|en|>", task="transcribe")
        assert isinstance(got, list) and len(got) == 2
        for a, (wt, ww) in zip(got, want):
            assert a["text"] == wt
            ok, why = Hh.words_equal(a["chunks"], ww, tol=0.0)
            assert ok, why
        one = pipe.align(clips[1], list(texts[1]), language="<|en|>")
        assert one["text"] == want[1][0]
        cw.adjust_pauses_for_hf_pipeline_output(one)
        det = pipe.align(clips, [[5, 6, 7], [8, 9]], language=None)
        assert len(det) == 2 and all("chunks" in d for d in det)
    finally:
        pipe.engine.close()


def test_align_tokens_refusals(tiny):
    g, v, W, spec = tiny
    eng = _engine(spec, W, "f32", rows=2)
    try:
        _, nf = eng.mel([syn.synth_audio(1, 16000 * 5, "mixed")])
        init = [v.sot, v.lang_id("en"), v.transcribe]
        ok = np.array(init + [5, 6, v.eos])
        assert len(eng.align_tokens(nf, [ok], 3)[0]) == 6
        import ctypes as C
        for bad in (g.vocab, -1):
            with pytest.raises(ValueError, match="vocabulary"):                # the wrapper, before an int32 table could wrap
                eng.align_tokens(nf, [np.array(init + [bad, v.eos])], 3)
            table = np.array([init + [bad, v.eos]], np.int32)
            n = np.array([5], np.int32)
            nfa = np.asarray(nf, np.int32)
            ts = np.zeros((1, 5), np.float32)
            p = lambda a: a.ctypes.data_as(C.c_void_p)
            assert eng.lib.cw_align_tokens(eng.ctx, 1, p(nfa), p(table), 5, p(n), 3, p(ts)) != 0
            assert b"vocabulary" in eng.lib.cw_last_error(eng.ctx)
        with pytest.raises(ValueError, match="vocabulary"):
            eng.align_tokens(nf, [np.array(init + [2 ** 32 + 5, v.eos])], 3)
        cases = [
            ([np.array(init)], 3, "ids"),
            ([np.array(init + [5] * (g.max_target_positions))], 3, "ids"),
            ([np.array(init + [5, v.eos, 6, v.eos])], 3, "eos"),
            ([ok, ok, ok], 3, "nb"),
        ]
        for ids, n_init, word in cases:
            with pytest.raises(EngineError, match=word):
                eng.align_tokens(np.resize(nf, len(ids)), ids, n_init)
        assert len(eng.align_tokens(nf, [ok], 3)[0]) == 6          # a refused call leaves the context usable
    finally:
        eng.close()
