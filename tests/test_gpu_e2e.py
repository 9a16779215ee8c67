"""GPU parity tests, path level: encoder / teacher-forced decoder / full pipeline through the C ABI
against the golden fixtures (transformers 5.15.0) and the oracle."""
import numpy as np
import pytest

import crisperwhisper_amd as cw
from crisperwhisper_amd import collate, generation, synthetic as syn
from crisperwhisper_amd.engine import Engine
from oracle import mel as OM
from oracle.model import WhisperOracle
from tests import helpers as Hh

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tiny():
    g, v, W, spec = Hh.tiny_setup()
    return g, v, W, spec


@pytest.fixture(scope="module")
def eng_f32(tiny):
    g, v, W, spec = tiny
    e = Engine(spec, dtype="f32", max_batch=4)
    e.load_state_dict(W)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_bf16(tiny):
    g, v, W, spec = tiny
    e = Engine(spec, dtype="bf16", max_batch=4)
    e.load_state_dict(W)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_f16(tiny):
    g, v, W, spec = tiny
    e = Engine(spec, dtype="f16", max_batch=4)
    e.load_state_dict(W)
    yield e
    e.close()


def _first_window_feats(g):
    x = syn.synth_audio(0, 70 * 16000, "mixed")[:480000]
    return OM.log_mel(x[None], g.n_mels)


def test_encoder_f32_vs_golden(tiny, eng_f32):
    g, v, W, spec = tiny
    z = Hh.gold_npz("e2e_golden.npz")
    eng_f32.set_features(_first_window_feats(g))
    eng_f32.encode([0], [0], [3000])
    enc = eng_f32.encoder_output(1)
    err = np.abs(enc[0][::10] - z["tf/enc_sub"]).max()
    assert err < 1e-3, err            # f32 mode: <= 1e-3 abs on O(1) activations


def test_encoder_seek_window_matches_oracle(tiny, eng_f32):
    """Window slicing inside the conv gather: seek/zero-pad semantics of _get_input_segment."""
    g, v, W, spec = tiny
    feats = _first_window_feats(g)
    eng_f32.set_features(feats)
    eng_f32.encode([0, 0], [0, 1000], [3000, 700])
    enc = eng_f32.encoder_output(2)
    seg = np.zeros((1, g.n_mels, 3000), np.float32); seg[0, :, :700] = feats[0, :, 1000:1700]
    ref = WhisperOracle(W, g).encode(seg)
    assert np.abs(enc[1] - ref[0]).max() < 1e-3


@pytest.mark.parametrize("mode", ["f32", "bf16", "f16"])
def test_teacher_forced_decoder(tiny, eng_f32, eng_bf16, eng_f16, mode):
    g, v, W, spec = tiny
    eng = {"f32": eng_f32, "bf16": eng_bf16, "f16": eng_f16}[mode]
    z = Hh.gold_npz("e2e_golden.npz")
    ids = z["tf/ids"]                                   # [1, 3 + 12]
    T = ids.shape[1]
    eng.set_features(_first_window_feats(g))
    eng.encode([0], [0], [3000])
    cap = eng.capture_logits(1, T)
    forced = np.full((1, T), -1, np.int32); forced[0, 3:] = ids[0, 3:]
    seqs, lens, amax = eng.decode(ids[:, :3], max_length=T, forced=forced, want_argmax=True)
    eng.stop_capture()
    assert seqs[0, :T].tolist() == ids[0].tolist()
    ref_logits = z["tf/logits"]                         # row t = logits after feeding ids[:t+1]
    got = cap[:T - 3, 0]                                # step s = logits used to choose token 3+s
    want = ref_logits[2:T - 1]
    if mode == "f32":
        assert np.abs(got - want).max() < 2e-3
    elif mode == "f16":
        assert np.abs(got - want).max() < 0.04          # binary16: 3 more significand bits than bfloat16
        assert (got.argmax(-1) == want.argmax(-1)).mean() >= 0.9
    else:
        assert np.abs(got - want).max() < 0.25          # bf16 weights/activations, logits std ~2
        assert (got.argmax(-1) == want.argmax(-1)).mean() >= 0.9
    al = eng.alignment(1, T - 1)                        # [1, Ha, T-1, 1500]
    # probability rows: f32 mode to 1e-5 abs; bf16 mode (bf16 q/K, f32 softmax) to 2e-2 abs on rows
    # whose peaks are O(0.1-1) -- the DTW input is z-scored so this is ~1e-2 relative
    tol = {"f32": 1e-5, "f16": 4e-3, "bf16": 2e-2}[mode]
    assert np.abs(al[0] - z["tf/cross"][:, :T - 1]).max() < tol
    assert np.abs(al[0].sum(-1) - 1).max() < 1e-3       # rows are probability vectors


@pytest.mark.parametrize("name", ["mixed70_b2_n40", "noise35_b4_free", "chirp12_b1_n24", "noise40_b2_autolang", "mixed20_b1_autolang_notask", "noise30_b1_maxlen", "noise_1sample", "noise_100ms"])
def test_pipeline_f32_word_for_word_vs_reference(tiny, name):
    """The drop-in call of REF/transcribe.py:21-33 + REF/README pause split, f32 engine, against the
    transformers CPU output: identical text/words, timestamps within +-0.02 s (one encoder frame)."""
    g, v, W, spec = tiny
    meta = Hh.gold_json("e2e_golden.json")[name]
    x = syn.synth_audio(meta["seed"], int(round(meta["secs"] * 16000)), meta["kind"])
    pipe = cw.pipeline("automatic-speech-recognition", model=cw.ModelBundle(spec, W),
                       tokenizer=collate.Vocabulary.from_synthetic(v), chunk_length_s=30,
                       batch_size=meta["batch_size"], return_timestamps="word", torch_dtype="float32", device="cuda:0")
    out = pipe(x, generate_kwargs={**Hh.GEN_KW, **meta["extra"]})
    assert out["text"] == meta["text"]
    ok, why = Hh.words_equal(out["chunks"], meta["chunks"], tol=0.02)
    assert ok, why
    pipe.engine.close()


def test_pipeline_bf16_runs_and_is_well_formed(tiny):
    g, v, W, spec = tiny
    x = syn.synth_audio(9, 50 * 16000, "mixed")
    pipe = cw.pipeline("automatic-speech-recognition", model=cw.ModelBundle(spec, W),
                       tokenizer=collate.Vocabulary.from_synthetic(v), chunk_length_s=30, batch_size=2,
                       return_timestamps="word", device="cuda:0")
    out = pipe(x, generate_kwargs={**Hh.GEN_KW, "max_new_tokens": 32, "min_new_tokens": 32})
    assert isinstance(out["text"], str) and len(out["chunks"]) > 0
    assert "".join(c["text"] for c in out["chunks"]) == out["text"]
    adj = cw.adjust_pauses_for_hf_pipeline_output(out)
    for a, b in zip(adj["chunks"][:-1], adj["chunks"][1:]):
        assert np.isfinite(a["timestamp"]).all() and np.isfinite(b["timestamp"]).all()
    pipe.engine.close()


@pytest.mark.parametrize("min_tiles", [200, 1])
def test_large_geometry_layers_bf16_vs_oracle(min_tiles):
    """min_tiles = 1 forces the 256x256 GEMM for every encoder GEMM (conv gather, HEADS / RESID / GELU epilogues).
    BASELINE-size shapes (d=1280, 20 heads, ffn 5120, vocab 51866, 15 alignment heads) on a 2+2-layer
    stack: exercises every large-shape kernel path of the bf16 engine (LDS-DMA GEMM tiles with M/N edges,
    K-split atomic GEMVs, 4-way split cross-attention + combine, 51866-wide logits + sampler) against the
    f32 oracle, teacher-forced.  Tolerances: bf16 weights/activations vs f32 reference."""
    g, v = syn.large_v3_geometry()
    g.enc_layers = g.dec_layers = 2
    spec = syn.model_spec(g, v, n_align=15)
    spec.alignment_heads = [[l, h] for l in range(2) for h in (0, 3, 7, 19)]
    W = syn.random_weights(g, seed=3)
    x = syn.synth_audio(11, 480000, "mixed")
    feats = OM.log_mel(x[None], g.n_mels)
    orc = WhisperOracle(W, g)
    enc_ref = orc.encode(feats)
    eng = Engine(spec, dtype="bf16", max_batch=2)
    eng.load_state_dict(W)
    eng.lib.cw_test_set_option(b"gemm256_min_tiles", min_tiles)
    try:
        f2, _ = eng.mel([x, x[:200000]], return_features=True)
        assert np.abs(f2[0] - feats[0]).max() < 1e-4
        eng.encode([0, 1], [0, 0], [3000, 1250])
        enc = eng.encoder_output(2)
        scale = np.abs(enc_ref).max()
        assert np.abs(enc[0] - enc_ref[0]).max() < 0.06 * scale, np.abs(enc[0] - enc_ref[0]).max() / scale
        # item 1: 200000 samples -> 1250 valid frames, zero-padded window (conv gather + seek-window semantics)
        xp, _ = OM.pad_or_trim(x[:200000])
        seg = np.zeros((1, g.n_mels, 3000), np.float32)
        seg[0, :, :1250] = OM.log_mel(xp[None], g.n_mels)[0, :, :1250]
        enc_ref1 = orc.encode(seg)
        assert np.abs(enc[1] - enc_ref1[0]).max() < 0.06 * np.abs(enc_ref1).max()
        # teacher-forced decode of 10 tokens on item 0 (batch row 1 rides along)
        T = 13
        rng = np.random.default_rng(0)
        ids = np.concatenate([[v.sot, v.lang_id("en"), v.transcribe], [v.timestamp_begin], rng.integers(300, 50000, T - 5), [v.timestamp_begin + 40]])[None]
        cache = orc.new_cache(enc_ref)
        ref_logits, ref_cross = orc.decode(ids, cache, want_heads=[list(h) for h in spec.alignment_heads], all_logits=True)
        cap = eng.capture_logits(2, T)
        forced = np.full((2, T), -1, np.int32); forced[:, 3:] = ids[0, 3:]
        seqs, lens, amax = eng.decode(np.tile(ids[:, :3], (2, 1)), max_length=T, forced=forced, want_argmax=True)
        eng.stop_capture()
        got, want = cap[:T - 3, 0], ref_logits[0, 2:T - 1]
        rel = np.abs(got - want).max() / np.abs(want).max()
        assert rel < 0.08, rel
        # the graph path (no capture) must give the same argmax trace as the eager path
        seqs2, lens2, amax2 = eng.decode(np.tile(ids[:, :3], (2, 1)), max_length=T, forced=forced, want_argmax=True)
        assert np.array_equal(amax[:, 3:T], amax2[:, 3:T])
        al = eng.alignment(1, T - 1)
        assert np.abs(al[0] - ref_cross[0][:, :T - 1]).max() < 3e-2
        assert np.abs(al[0].sum(-1) - 1).max() < 2e-3
        ts = eng.token_timestamps(2, T - 1, 3, [3000, 1250])
        assert np.isfinite(ts).all() and (ts[:, 3:] >= 0).all() and (ts[0] <= 30.0).all() and (ts[1] <= 12.5 + 1e-6).all()
    finally:
        eng.lib.cw_test_set_option(b"gemm256_min_tiles", 200)
        eng.close()


def test_reference_call_sequence_with_hf_objects_and_wav_path(tiny, tmp_path):
    """Literally REF/transcribe.py:14-33 with `pipeline` swapped for ours: HF model + processor objects in,
    a .wav path in, the reference's result dict out; then REF/README's adjust_pauses call."""
    transformers = pytest.importorskip("transformers")
    import torch
    from scipy.io import wavfile
    from tests.golden import hf_synth as H
    g, v, W, spec = tiny
    model = H.build_model(g, v, n_align=3)
    sd = {k: torch.from_numpy(x) for k, x in W.items()}
    sd["proj_out.weight"] = sd["model.decoder.embed_tokens.weight"]
    model.load_state_dict(sd, strict=True)
    model.generation_config.alignment_heads = syn.alignment_heads(g, 3)
    tok, fe = H.build_tokenizer(v), H.build_feature_extractor(g)
    meta = Hh.gold_json("e2e_golden.json")["mixed70_b2_n40"]
    x = syn.synth_audio(meta["seed"], int(round(meta["secs"] * 16000)), meta["kind"])
    path = str(tmp_path / "clip.wav")
    wavfile.write(path, 16000, x)                                  # float32 WAV: lossless
    pipe = cw.pipeline("automatic-speech-recognition", model=model, tokenizer=tok, feature_extractor=fe,
                       chunk_length_s=30, batch_size=2, return_timestamps="word", torch_dtype=torch.float32,
                       device="cuda:0")
    out = pipe(path, generate_kwargs={**Hh.GEN_KW, **meta["extra"]})
    assert out["text"] == meta["text"]
    ok, why = Hh.words_equal(out["chunks"], meta["chunks"], tol=0.02)
    assert ok, why
    out2 = pipe({"array": x, "sampling_rate": 16000}, generate_kwargs={**Hh.GEN_KW, **meta["extra"]})
    assert out2 == out
    from oracle import pauses as OP
    import copy
    want = OP.adjust_pauses_for_hf_pipeline_output(copy.deepcopy(out))
    got = cw.adjust_pauses_for_hf_pipeline_output(out)
    assert got is out and got == want
    with pytest.raises(ValueError):
        pipe({"array": x})                                         # missing sampling_rate, like the reference
    with pytest.raises(TypeError):
        pipe(12345)
    pipe.engine.close()


def test_ten_minute_long_form_vs_oracle(tiny):
    """BASELINE configs[2] on one GPU: 600 s stream -> 30 chunks (29 x 30 s + 20 s, 5 s strides), batch_size 16,
    seam merge across all chunk boundaries; tiny f32 engine vs the oracle pipeline (pinned to transformers)."""
    from oracle import pipeline as OPIPE
    g, v, W, spec = tiny
    x = np.concatenate([syn.synth_audio(100 + i, 16000 * 60, "mixed" if i % 2 else "noise") for i in range(10)])
    assert len(x) == 9_600_000
    pipe = cw.pipeline("automatic-speech-recognition", model=cw.ModelBundle(spec, W),
                       tokenizer=collate.Vocabulary.from_synthetic(v), chunk_length_s=30, batch_size=16,
                       return_timestamps="word", torch_dtype="float32", device="cuda:0")
    kw = {**Hh.GEN_KW, "max_new_tokens": 24}
    out = pipe(x, generate_kwargs=kw)
    want = OPIPE.transcribe(WhisperOracle(W, g), Hh.oracle_spec(g, v, spec), Hh.oracle_vocab(v), x, n_mels=g.n_mels,
                            batch_size=16, max_new_tokens=24)
    assert out["text"] == want["text"]
    ok, why = Hh.words_equal(out["chunks"], want["chunks"], tol=0.02)
    assert ok, why
    assert len(out["chunks"]) > 30
    pipe.engine.close()


def test_concurrent_contexts_give_identical_result(tiny):
    """pipeline(contexts=2): alternate batches run on two engine contexts from two host threads; chunks are
    independent, so the merged result must equal the single-context one (f32 engine: bit-identical tokens)."""
    g, v, W, spec = tiny
    x = syn.synth_audio(21, 130 * 16000, "mixed")
    kw = {**Hh.GEN_KW, "max_new_tokens": 20}
    outs = []
    for contexts in (1, 2):
        pipe = cw.pipeline("automatic-speech-recognition", model=cw.ModelBundle(spec, W),
                           tokenizer=collate.Vocabulary.from_synthetic(v), chunk_length_s=30, batch_size=2,
                           return_timestamps="word", torch_dtype="float32", device="cuda:0", contexts=contexts)
        outs.append(pipe(x, generate_kwargs=kw))
        for e in pipe.engines:
            e.close()
    assert outs[0] == outs[1] and len(outs[0]["chunks"]) > 0


@pytest.mark.parametrize("seed", [101, 202, 303])
def test_live_transformers_pipeline_parity_on_fresh_inputs(seed):
    """Not a fixture: fresh random weights + audio per seed, the installed transformers pipeline on the host CPU
    (the reference's exact call, REF/transcribe.py:21-33) vs the native pipeline (f32 engine) on the GPU."""
    pytest.importorskip("transformers")
    import torch
    from tests.golden import hf_synth as H
    g, v = syn.tiny_geometry()
    W = syn.random_weights(g, seed=seed)
    spec = syn.model_spec(g, v, 3)
    model = H.build_model(g, v, n_align=3)
    sd = {k: torch.from_numpy(x) for k, x in W.items()}
    sd["proj_out.weight"] = sd["model.decoder.embed_tokens.weight"]
    model.load_state_dict(sd, strict=True)
    model.generation_config.alignment_heads = syn.alignment_heads(g, 3)
    tok, fe = H.build_tokenizer(v), H.build_feature_extractor(g)
    rng = np.random.default_rng(seed)
    secs = int(rng.integers(8, 75))
    x = syn.synth_audio(seed, secs * 16000, ["noise", "mixed", "chirp"][seed % 3])
    bs = int(rng.integers(1, 4))
    kw = {**Hh.GEN_KW, "max_new_tokens": int(rng.integers(12, 48))}
    ref = H.build_pipeline(model, tok, fe, batch_size=bs)(x.copy(), generate_kwargs=kw)
    pipe = cw.pipeline("automatic-speech-recognition", model=model, tokenizer=tok, feature_extractor=fe,
                       chunk_length_s=30, batch_size=bs, return_timestamps="word", torch_dtype=torch.float32,
                       device="cuda:0")
    out = pipe(x, generate_kwargs=kw)
    pipe.engine.close()
    assert out["text"] == ref["text"]
    ok, why = Hh.words_equal(out["chunks"], [{"text": c["text"], "timestamp": list(c["timestamp"])} for c in ref["chunks"]], tol=0.02)
    assert ok, why


@pytest.mark.parametrize("language,task,kw", [
    ("<|en|>", "transcribe", dict(max_new_tokens=40)),
    ("<|en|>", "transcribe", dict()),
    (None, None, dict(max_new_tokens=24)),
    (None, "transcribe", dict(max_new_tokens=24, min_new_tokens=8)),
])
def test_native_seek_loop_equals_host_loop(tiny, eng_f32, language, task, kw):
    """cw_transcribe (seek loop inside the library) against the stage-by-stage host loop in generation.generate:
    identical token ids and bit-identical token timestamps, same number of passes."""
    from crisperwhisper_amd import generation
    g, v, W, spec = tiny
    clips = [syn.synth_audio(60 + i, n, kind) for i, (n, kind) in
             enumerate([(480000, "mixed"), (130000, "noise"), (300001, "chirp"), (1600, "noise")])]
    _, nf = eng_f32.mel(clips)
    sa, sb = {}, {}
    a = generation.generate(eng_f32, len(clips), nf, language=language, task=task, stats=sa, native=True, **kw)
    b = generation.generate(eng_f32, len(clips), nf, language=language, task=task, stats=sb, native=False, **kw)
    assert sa == sb
    assert np.array_equal(a["sequences"], b["sequences"])
    for x, y in zip(a["token_timestamps"], b["token_timestamps"]):
        assert x.dtype == np.float32 and np.array_equal(x, y)


@pytest.mark.parametrize("skinny_mode", [0, 1, 2])
def test_large_batch_decode_matches_small_batch_path(request, skinny_mode):
    """Decode batches of 17..64 rows take the one-weight-pass GEMV (prep + multi-tile kernel, gemm.hip); batches of
    <= 16 rows the latency kernel.  Same engine, same 20 windows, large-v3 shapes (K-split atomics, combine, 51866
    logits): teacher-forced logits of the two paths agree to bf16 rounding and pick the same tokens.
    skinny_mode 0 (default): the round-3 path.  1: cross-attention query through K-split planes finished inside the one-block-per-(row, head)
    cross-attention, which writes the out-projection's rows; 2: every LayerNorm projection through
    csrc/skinny.hip planes + finish launch.  Modes 1 and 2 were measured slower in the step and live in -DCW_EXPERIMENTS builds."""
    if skinny_mode and not Hh.has_experiments():     # A/B kernel variants: -DCW_EXPERIMENTS builds
        return Hh.run_in_child(request, Hh.experiments_env(), lambda p: p["skinny_mode"] != 0)
    g, v = syn.large_v3_geometry()
    g.enc_layers = g.dec_layers = 2
    spec = syn.model_spec(g, v, n_align=15)
    spec.alignment_heads = [[l, h] for l in range(2) for h in (0, 3, 7, 19)]
    W = syn.random_weights(g, seed=5)
    B, T = 20, 9
    clips = [syn.synth_audio(200 + i, 480000 - 20000 * i, ("noise", "chirp", "mixed")[i % 3]) for i in range(B)]
    rng = np.random.default_rng(1)
    ids = np.concatenate([[v.sot, v.lang_id("en"), v.transcribe], [v.timestamp_begin], rng.integers(300, 50000, T - 4)])
    forced = np.full((B, T), -1, np.int32); forced[:, 3:] = ids[3:]
    prompt = np.tile(ids[None, :3], (B, 1))
    eng = Engine(spec, dtype="bf16", max_batch=B)
    eng.load_state_dict(W)
    try:
        eng._chk(eng.lib.cw_set_option(eng.ctx, b"skinny", skinny_mode))
        eng.mel(clips)
        eng.encode(list(range(B)), [0] * B, [3000] * B)
        cap = eng.capture_logits(B, T)
        eng.decode(prompt, max_length=T, forced=forced)
        big = cap[:T - 3].copy()
        al_big = eng.alignment(B, T - 1)
        eng.stop_capture()
        for lo in (0, 10):
            items = list(range(lo, lo + 10))
            eng.encode(items, [0] * 10, [3000] * 10)
            cap = eng.capture_logits(10, T)
            eng.decode(prompt[:10], max_length=T, forced=forced[:10])
            small = cap[:T - 3].copy()
            al_small = eng.alignment(10, T - 1)
            eng.stop_capture()
            ref = small
            got = big[:, lo:lo + 10]
            rel = np.abs(got - ref).max() / np.abs(ref).max()
            same = got.argmax(-1) == ref.argmax(-1)
            top2 = np.sort(ref, axis=-1)[..., -2:]
            clear = (top2[..., 1] - top2[..., 0]) > 2.0 * np.abs(got - ref).max(-1)   # margin beyond the two paths' rounding noise
            assert rel < 0.03, rel
            assert same[clear].all() and clear.mean() > 0.5, (float(same.mean()), float(clear.mean()))
            assert same.mean() >= 0.9, float(same.mean())       # random weights: near-flat logits, a few positions are toss-ups
            assert np.abs(al_big[lo:lo + 10] - al_small).max() < 2e-2
    finally:
        eng.close()


@pytest.mark.parametrize("name", ["large_mixed30_n32", "large_noise12_n24", "large_mixed70_b2_n20", "large_beam5_mixed30_n16",
                                  "large_beam3_noise45_b2_n12_autolang"])
def test_full_size_f32_pipeline_word_for_word_vs_transformers(name):
    """BASELINE geometry end to end (large-v3 shapes, 32 + 32 layers, vocab 51866, 15 alignment heads, 1.54 B synthetic
    parameters): the reference pipeline call through the f32 engine against the committed transformers 5.15.0 CPU
    output (tests/golden/gen_golden_large.py): identical text and words, timestamps within one encoder frame."""
    import os
    path = os.path.join(os.path.dirname(__file__), "golden", "e2e_large_golden.json")
    if not os.path.exists(path):
        pytest.skip("full-size golden not generated")
    meta = Hh.gold_json("e2e_large_golden.json")[name]
    g, v = syn.large_v3_geometry()
    spec = syn.model_spec(g, v, n_align=15)
    x = syn.synth_audio(meta["seed"], int(round(meta["secs"] * 16000)), meta["kind"])

    class LazyWeights(dict):                      # stream the 6.2 GB of f32 weights tensor by tensor
        def items(self):
            for n, shape in syn.weight_shapes(g).items():
                yield n, syn.random_tensor(g, n, shape, seed=meta["weight_seed"])
    pipe = cw.pipeline("automatic-speech-recognition", model=cw.ModelBundle(spec, LazyWeights()),
                       tokenizer=collate.Vocabulary.from_synthetic(v), chunk_length_s=30, batch_size=meta.get("batch_size", 1),
                       return_timestamps="word", torch_dtype="float32", device="cuda:0")
    try:
        out = pipe(x, generate_kwargs=dict(meta["generate_kwargs"]))
        assert out["text"] == meta["text"]
        ok, why = Hh.words_equal(out["chunks"], meta["chunks"], tol=0.02)
        assert ok, why
    finally:
        pipe.engine.close()


def test_full_size_bf16_engine_tracks_f32_engine():
    """Performance mode against parity mode at the BASELINE geometry (32 + 32 layers): the f32 engine (word-for-word
    with transformers, test above) decodes a window greedily; the bf16 engine is teacher-forced on those tokens.
    Stated accuracy of the bf16 path at full depth: logits within 3 % of the logit range, >= 90 % top-1 agreement,
    alignment rows within 3e-2, token timestamps within one encoder frame on >= 80 % of the tokens (measured 87.5 %:
    random weights give near-uniform alignment rows, so the DTW path is far more fragile here than with trained heads)."""
    g, v = syn.large_v3_geometry()
    spec = syn.model_spec(g, v, n_align=15)
    x = syn.synth_audio(21, 480000, "mixed")
    engs = {}
    try:
        for dt in ("f32", "bf16"):
            engs[dt] = Engine(spec, dtype=dt, max_batch=1)
        for n, shape in syn.weight_shapes(g).items():
            w = syn.random_tensor(g, n, shape, seed=0)
            for e in engs.values():
                e.load_tensor(n, w)
        prompt = np.array([[v.sot, v.lang_id("en"), v.transcribe]], np.int32)
        T = 3 + 40
        res = {}
        forced = None
        for dt in ("f32", "bf16"):
            e = engs[dt]
            e.mel([x])
            e.encode([0], [0], [3000])
            cap = e.capture_logits(1, T)
            seqs, lens, amax = e.decode(prompt, max_length=T, min_new_tokens=40, forced=forced, want_argmax=True)
            e.stop_capture()
            n = int(lens[0])
            if forced is None:
                forced = np.full((1, T), -1, np.int32); forced[0, 3:n] = seqs[0, 3:n]
            res[dt] = dict(n=n, logits=cap[:n - 3, 0].copy(), amax=amax[0, 3:n].copy(), al=e.alignment(1, n - 1)[0],
                           ts=e.token_timestamps(1, n - 1, 3, [3000])[0], enc=e.encoder_output(1)[0])
        a, b = res["f32"], res["bf16"]
        assert a["n"] == b["n"] == T
        enc_rel = np.abs(a["enc"] - b["enc"]).max() / np.abs(a["enc"]).max()
        assert enc_rel < 0.08, enc_rel
        rng_ = a["logits"].max() - a["logits"].min()
        assert np.abs(a["logits"] - b["logits"]).max() < 0.03 * rng_, np.abs(a["logits"] - b["logits"]).max() / rng_
        assert (a["amax"] == b["amax"]).mean() >= 0.9, (a["amax"] == b["amax"]).mean()
        assert np.abs(a["al"] - b["al"]).max() < 3e-2, np.abs(a["al"] - b["al"]).max()
        close = np.abs(a["ts"][3:] - b["ts"][3:]) <= 0.02 + 1e-6
        assert close.mean() >= 0.8 and np.median(np.abs(a["ts"][3:] - b["ts"][3:])) == 0.0, (close.mean(), a["ts"], b["ts"])
    finally:
        for e in engs.values():
            e.close()


def _aligned_weights(g, seed=0):
    class Lazy(dict):                               # stream the 6.2 GB of f32 tensors one at a time
        def items(self):
            for n, shape in syn.weight_shapes(g).items():
                yield n, syn.weight_tensor(g, n, shape, seed, "aligned")
    return Lazy()


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_bench_shape_bf16_timestamps_and_words_vs_transformers(dtype):
    """Parity of the TIMED path at the TIMED shape (BASELINE configs[1] = what bench.py runs): bf16 engine, large-v3
    geometry (32 + 32 layers), B = 8 x 30 s clips in one batch, 128 tokens per generate pass -- against the reference
    pipeline run through transformers 5.15.0 on the CPU in fp32 (tests/golden/gen_golden_bench.py), teacher-forced on
    the reference's tokens pass by pass of the seek loop.

    Weights: the *aligned* synthetic set (crisperwhisper_amd.synthetic.aligned_tensor) -- seeded random tensors whose 15
    alignment heads are peaked and monotone, as a trained checkpoint's are; with i.i.d. random weights every attention
    row is near-uniform and the z-score amplifies any rounding into a different DTW path (that case is
    test_full_size_bf16_engine_tracks_f32_engine, stated there).

    Bars (north_star): token timestamps within +-0.02 s of the reference on >= 99 % of the generated tokens of every
    pass; after the reference's own segment slicing and word collation of those tokens with OUR timestamps, the text is
    identical and >= 99 % of the words are within +-0.02 s at both ends."""
    import os
    from crisperwhisper_amd import generation
    path = os.path.join(os.path.dirname(__file__), "golden", "e2e_bench_golden.json")
    if not os.path.exists(path):
        pytest.skip("bench-shape golden not generated")
    gold = Hh.gold_json("e2e_bench_golden.json")
    clips_g = gold["clips"]
    B = len(clips_g)
    assert B == 8
    g, v = syn.large_v3_geometry()
    spec = syn.model_spec(g, v, n_align=15)
    n_tok = gold["generate_kwargs"]["max_new_tokens"]
    clips = [syn.synth_audio(c["seed"], 480000, c["kind"]) for c in clips_g]
    tb = v.timestamp_begin
    n_prompt = 3
    T = n_prompt + n_tok
    eng = Engine(spec, dtype=dtype, max_batch=B)
    try:
        eng.load_state_dict(_aligned_weights(g, gold["weight_seed"]))
        _, nf = eng.mel(clips)
        assert nf.tolist() == [3000] * B
        prompt = np.tile(np.array([[v.sot, v.lang_id("en"), v.transcribe]], np.int32), (B, 1))
        n_tokens = n_close = 0
        worst = 0.0
        ours = [[] for _ in range(B)]                       # per clip: [(golden ids of the pass, our timestamps)]
        # ---- pass 1: all 8 windows in one batch, exactly the bench's first decode call
        p0 = [c["passes"][0] for c in clips_g]
        assert all(p["num_frames"] == [3000] and len(p["sequences"][0]) == T for p in p0)
        forced = np.full((B, T), -1, np.int32)
        for i, p in enumerate(p0):
            assert p["sequences"][0][:n_prompt] == prompt[i].tolist()
            forced[i, n_prompt:] = p["sequences"][0][n_prompt:]
        eng.encode(list(range(B)), [0] * B, [3000] * B)
        seqs, lens, amax = eng.decode(prompt, max_length=T, min_new_tokens=n_tok, forced=forced, want_argmax=True)
        assert lens.tolist() == [T] * B
        ts = eng.token_timestamps(B, T - 1, n_prompt, [3000] * B)
        agree = float((amax[:, n_prompt:T] == forced[:, n_prompt:T]).mean())
        for i, p in enumerate(p0):
            want = np.asarray(p["token_timestamps"][0], np.float64)
            d = np.abs(ts[i, n_prompt:T] - want[n_prompt:T])
            n_tokens += d.size; n_close += int((d <= 0.02 + 1e-6).sum()); worst = max(worst, float(d.max()))
            ours[i].append((np.asarray(p["sequences"][0], np.int64), ts[i].copy(), 0))
        # ---- later passes of the seek loop: one window per call, like the reference's batch_size = 1 run
        for i, c in enumerate(clips_g):
            for p in c["passes"][1:]:
                nfi = int(p["num_frames"][0])
                seek = 3000 - nfi
                f1 = np.full((1, T), -1, np.int32); f1[0, n_prompt:] = p["sequences"][0][n_prompt:]
                eng.encode([i], [seek], [3000 - seek])
                eng.decode(prompt[:1], max_length=T, min_new_tokens=n_tok, forced=f1)
                t1 = eng.token_timestamps(1, T - 1, n_prompt, [nfi])
                want = np.asarray(p["token_timestamps"][0], np.float64)
                d = np.abs(t1[0, n_prompt:T] - want[n_prompt:T])
                n_tokens += d.size; n_close += int((d <= 0.02 + 1e-6).sum()); worst = max(worst, float(d.max()))
                ours[i].append((np.asarray(p["sequences"][0], np.int64), t1[0].copy(), seek))
        frac = n_close / n_tokens
        print(f"bench-shape {dtype} parity: {n_close}/{n_tokens} token timestamps within 0.02 s ({100 * frac:.2f} %), worst {worst:.2f} s, "
              f"free-running top-1 agreement under teacher forcing {100 * agree:.1f} %")
        assert frac >= 0.99, (frac, worst)
        # ---- words: the reference's segment slicing (generation_whisper.py:1977-2074) + _decode_asr on the reference
        # tokens with the bf16 engine's timestamps
        vocab = collate.Vocabulary.from_synthetic(v)
        n_words = n_words_close = 0
        for i, c in enumerate(clips_g):
            toks, tts = [], []
            for ids, t_, seek in ours[i]:
                s_ = ids[n_prompt:]
                if s_[-1] == v.eos:
                    s_ = s_[:-1]
                segs, adv = generation.split_segments(s_, t_, float(seek) * 0.02 / 2, tb, 3000 - seek, n_prompt)
                for sg in segs:
                    toks.append(sg.tokens); tts.append(sg.token_timestamps)
            toks = np.concatenate(toks); tts = np.concatenate(tts)
            text, words = collate.decode_asr(vocab, [{"tokens": toks, "token_timestamps": tts, "stride": (30.0, 0.0, 0.0)}])
            assert text == c["text"], i
            assert [w["text"] for w in words] == [w["text"] for w in c["chunks"]], i
            for a, b in zip(words, c["chunks"]):
                n_words += 1
                n_words_close += int(all(abs(x - y) <= 0.02 + 1e-9 for x, y in zip(a["timestamp"], b["timestamp"])))
        print(f"bench-shape bf16 parity: {n_words_close}/{n_words} words within 0.02 s")
        assert n_words_close >= 0.99 * n_words, (n_words_close, n_words)
        # ---- informational: the untouched bench path (free-running greedy bf16, native seek loop) against the same golden
        out = generation.generate(eng, B, nf, language="<|en|>", task="transcribe", max_new_tokens=n_tok, min_new_tokens=n_tok)
        same_text = same_words = tot_words = 0
        for i, c in enumerate(clips_g):
            n = len(out["token_timestamps"][i])
            text, words = collate.decode_asr(vocab, [{"tokens": out["sequences"][i][:n], "token_timestamps": out["token_timestamps"][i],
                                                      "stride": (30.0, 0.0, 0.0)}])
            same_text += int(text == c["text"])
            if text == c["text"]:
                for a, b in zip(words, c["chunks"]):
                    tot_words += 1
                    same_words += int(all(abs(x - y) <= 0.02 + 1e-9 for x, y in zip(a["timestamp"], b["timestamp"])))
        print(f"bench-shape bf16 FREE-RUNNING: {same_text}/{B} clips reproduce the reference text, {same_words}/{tot_words} of their words within 0.02 s")
        # the path bench.py times, held to the reference: every clip's text, >= 99 % of the words within one frame
        assert same_text == B, (same_text, B)
        assert same_words >= 0.99 * tot_words and tot_words == sum(len(c["chunks"]) for c in clips_g), (same_words, tot_words)
        # BASELINE configs[5] harness (crisperwhisper_amd/metrics.py) on real pipeline output: boundary F1 at the 0.2 s collar and
        # mean word IoU of the free-running bf16 transcript against the reference transcript of clip 0
        from crisperwhisper_amd import metrics
        n0 = len(out["token_timestamps"][0])
        _, words0 = collate.decode_asr(vocab, [{"tokens": out["sequences"][0][:n0], "token_timestamps": out["token_timestamps"][0],
                                                "stride": (30.0, 0.0, 0.0)}])
        pr_, rc_, f1_ = metrics.boundary_f1(clips_g[0]["chunks"], words0, 0.2)
        iou_ = metrics.mean_iou(clips_g[0]["chunks"], words0)
        assert f1_ >= 0.99 and iou_ >= 0.9, (pr_, rc_, f1_, iou_)
        try:                                                # measured numbers for DESIGN.md (pulled back from the GPU box)
            import json
            os.makedirs("gpurun_out", exist_ok=True)
            json.dump({"tokens_within_20ms": n_close, "tokens": n_tokens, "worst_s": worst, "words_within_20ms": n_words_close,
                       "words": n_words, "teacher_forced_top1_agreement": agree, "free_running_clips_same_text": same_text,
                       "free_running_words_within_20ms": [same_words, tot_words]}, open(f"gpurun_out/parity_bench_shape_{dtype}.json", "w"))
        except OSError:
            pass
    finally:
        eng.close()


def test_fp8_cross_kv_cache_tracks_bf16_cache():
    """Opt-in e4m3 cross-attention cache (cw_set_option "cross_kv_fp8") against the bf16 cache of the same engine
    build, large-v3 shapes on a 2 + 2 layer stack, teacher-forced: the accuracy gate of that mode.  Logits within
    4 % of the logit range, >= 90 % top-1 agreement, alignment rows within 0.1 abs and correlated > 0.99 (3-bit mantissa
    keys move individual probabilities by a few percent); the f32 engine refuses the option."""
    g, v = syn.large_v3_geometry()
    g.enc_layers = g.dec_layers = 2
    spec = syn.model_spec(g, v, n_align=15)
    spec.alignment_heads = [[l, h] for l in range(2) for h in (0, 3, 7, 19)]
    W = syn.random_weights(g, seed=7)
    clips = [syn.synth_audio(300 + i, 480000 - 60000 * i, ("mixed", "noise", "chirp")[i]) for i in range(3)]
    T = 3 + 24
    prompt = np.tile(np.array([[v.sot, v.lang_id("en"), v.transcribe]], np.int32), (3, 1))
    res = {}
    forced = None
    for kv in (None, "fp8"):
        e = Engine(spec, dtype="bf16", max_batch=3, cross_kv_dtype=kv)
        try:
            e.load_state_dict(W)
            e.mel(clips)
            e.encode([0, 1, 2], [0, 0, 0], [3000, 3000, 3000])
            cap = e.capture_logits(3, T)
            seqs, lens, amax = e.decode(prompt, max_length=T, min_new_tokens=24, forced=forced, want_argmax=True)
            e.stop_capture()
            if forced is None:
                forced = np.full((3, T), -1, np.int32); forced[:, 3:] = seqs[:, 3:T]
            res[kv] = dict(logits=cap[:T - 3].copy(), amax=amax[:, 3:T].copy(), al=e.alignment(3, T - 1))
            # the graph path must agree with the eager (capture) path in this mode too
            seqs2, _, amax2 = e.decode(prompt, max_length=T, min_new_tokens=24, forced=forced, want_argmax=True)
            assert (amax2[:, 3:T] == res[kv]["amax"]).mean() >= 0.95
        finally:
            e.close()
    a, b = res[None], res["fp8"]
    rng_ = a["logits"].max() - a["logits"].min()
    assert np.abs(a["logits"] - b["logits"]).max() < 0.04 * rng_, np.abs(a["logits"] - b["logits"]).max() / rng_
    assert (a["amax"] == b["amax"]).mean() >= 0.9, (a["amax"] == b["amax"]).mean()
    assert np.abs(a["al"] - b["al"]).max() < 0.1, np.abs(a["al"] - b["al"]).max()
    cc = np.corrcoef(a["al"].ravel(), b["al"].ravel())[0, 1]
    assert cc > 0.99, cc
    assert np.abs(b["al"].sum(-1) - 1).max() < 2e-3
    with pytest.raises(Exception):
        Engine(spec, dtype="f32", max_batch=1, cross_kv_dtype="fp8")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_fp8_encoder_gemm_mode_tracks_bf16_engine(dt):
    """Opt-in e4m3 encoder mode (cw_set_option "encoder_gemm_fp8": qkv / fc1 / fc2 and the cross-K/V projections as
    v_mfma_scale_f32_16x16x128_f8f6f4 GEMMs, row-wise scales, LayerNorm-fused activation quantisation) against the bf16 GEMMs
    of the same engine, large-v3 shapes on a 4 + 2 layer stack, teacher-forced -- the accuracy gate of that mode: encoder
    states within 10 % relative L2 (3-bit mantissas on both operands of three GEMMs per layer: ~4 % noise per GEMM output on
    Gaussian data, measured 7 % after 4 layers), logits within 6 % of the logit range (measured 2.5 %), >= 85 % top-1 agreement (94 %),
    alignment rows correlated > 0.95 (0.972); switching the mode off restores the bf16 results bit for
    bit; the f32 engine refuses the option."""
    g, v = syn.large_v3_geometry()
    g.enc_layers, g.dec_layers = 4, 2
    spec = syn.model_spec(g, v, n_align=15)
    spec.alignment_heads = [[l, h] for l in range(2) for h in (0, 3, 7, 19)]
    W = syn.random_weights(g, seed=11)
    clips = [syn.synth_audio(400 + i, 480000 - 50000 * i, ("mixed", "noise", "chirp")[i]) for i in range(3)]
    T = 3 + 24
    prompt = np.tile(np.array([[v.sot, v.lang_id("en"), v.transcribe]], np.int32), (3, 1))
    e = Engine(spec, dtype=dt, max_batch=3)
    res = []
    try:
        e.load_state_dict(W)
        forced = None
        for mode in (False, True, False):
            e.set_encoder_gemm_fp8(mode)
            e.mel(clips)
            e.encode([0, 1, 2], [0, 0, 0], [3000, 3000, 3000])
            enc = e.encoder_output(3)
            cap = e.capture_logits(3, T)
            seqs, lens, amax = e.decode(prompt, max_length=T, min_new_tokens=24, forced=forced, want_argmax=True)
            e.stop_capture()
            if forced is None:
                forced = np.full((3, T), -1, np.int32); forced[:, 3:] = seqs[:, 3:T]
            res.append(dict(enc=enc.copy(), logits=cap[:T - 3].copy(), amax=amax[:, 3:T].copy(), al=e.alignment(3, T - 1)))
    finally:
        e.close()
    a, b, a2 = res
    assert np.array_equal(a["enc"], a2["enc"]) and np.array_equal(a["logits"], a2["logits"])      # mode off = the bf16 path again
    rel = float(np.linalg.norm(a["enc"] - b["enc"]) / np.linalg.norm(a["enc"]))
    rng_ = a["logits"].max() - a["logits"].min()
    dl = float(np.abs(a["logits"] - b["logits"]).max() / rng_)
    top1 = float((a["amax"] == b["amax"]).mean())
    cc = float(np.corrcoef(a["al"].ravel(), b["al"].ravel())[0, 1])
    print(f"fp8 encoder mode: encoder rel L2 {rel:.4f}, logits max diff / range {dl:.4f}, top-1 agreement {top1:.3f}, alignment corr {cc:.4f}")
    assert 1e-4 < rel < 0.10, rel                                                                  # really another path, and close
    assert dl < 0.06, dl                                                                          # measured 0.025
    assert top1 >= 0.85, top1                                                                     # measured 0.944
    assert cc > 0.95, cc                                                                          # measured 0.972
    with pytest.raises(Exception):
        e32 = Engine(spec, dtype="f32", max_batch=1)
        try:
            e32.load_state_dict(W)
            e32.set_encoder_gemm_fp8(True)
        finally:
            e32.close()


@pytest.mark.parametrize("name", ["mixed70_b2_n40", "noise35_b4_free", "chirp12_b1_n24"])
def test_pipeline_segment_timestamps_vs_reference(tiny, name):
    """return_timestamps=True (segment-level chunks, what REF/app.py:51-61 constructs its pipeline with), f32 engine,
    against the transformers CPU output: identical text, chunk texts and chunk timestamps."""
    g, v, W, spec = tiny
    meta = Hh.gold_json("e2e_segments_golden.json")[name]
    x = syn.synth_audio(meta["seed"], int(round(meta["secs"] * 16000)), meta["kind"])
    pipe = cw.pipeline("automatic-speech-recognition", model=cw.ModelBundle(spec, W),
                       tokenizer=collate.Vocabulary.from_synthetic(v), chunk_length_s=30,
                       batch_size=meta["batch_size"], return_timestamps=True, torch_dtype="float32", device="cuda:0")
    try:
        out = pipe(x, generate_kwargs={**Hh.GEN_KW, **meta["extra"]})
        assert out["text"] == meta["text"]
        assert [(c["text"], list(c["timestamp"])) for c in out["chunks"]] == [(c["text"], c["timestamp"]) for c in meta["chunks"]]
        out_w = pipe(x, return_timestamps="word", generate_kwargs={**Hh.GEN_KW, **meta["extra"]})     # per-call override (REF/app.py:102)
        assert out_w["text"] == Hh.gold_json("e2e_golden.json")[name]["text"]    # (seam merging differs between the two modes)
        with pytest.raises(ValueError):
            pipe(x, return_timestamps=False)
    finally:
        pipe.engine.close()


def test_pipeline_from_checkpoint_directory_without_transformers_objects(tiny, tmp_path):
    """`pipeline(model="<local snapshot dir>")`: config / generation config / safetensors / tokenizer.json read natively
    (the snapshot is written by transformers' save_pretrained), f32 engine, word for word against the golden."""
    pytest.importorskip("transformers")
    import torch
    from tests.golden import hf_synth as H
    g, v, W, spec = tiny
    model = H.build_model(g, v, n_align=3)
    sd = {k: torch.from_numpy(x) for k, x in W.items()}
    sd["proj_out.weight"] = sd["model.decoder.embed_tokens.weight"]
    model.load_state_dict(sd, strict=True)
    model.generation_config.alignment_heads = syn.alignment_heads(g, 3)
    d = str(tmp_path / "ckpt")
    model.save_pretrained(d); H.build_tokenizer(v).save_pretrained(d); H.build_feature_extractor(g).save_pretrained(d)
    meta = Hh.gold_json("e2e_golden.json")["mixed70_b2_n40"]
    x = syn.synth_audio(meta["seed"], int(round(meta["secs"] * 16000)), meta["kind"])
    pipe = cw.pipeline("automatic-speech-recognition", model=d, chunk_length_s=30, batch_size=meta["batch_size"],
                       return_timestamps="word", torch_dtype="float32", device="cuda:0")
    try:
        out = pipe(x, generate_kwargs={**Hh.GEN_KW, **meta["extra"]})
        assert out["text"] == meta["text"]
        ok, why = Hh.words_equal(out["chunks"], meta["chunks"], tol=0.02)
        assert ok, why
    finally:
        pipe.engine.close()


def test_bf16_engine_is_bit_reproducible_run_to_run():
    """The bf16 engine accumulates K-split GEMV partials into the residual stream with f32 atomics; the stream lives on
    a 2^-12 grid (common.h: resid_grid) so those additions are exact and their order cannot matter.  Large-v3 shapes
    (K-split 2 and 4 active), 8 rows, 48 free-running greedy steps, three runs (+ one on a second context): identical
    token ids and bit-identical logits of every step."""
    g, v = syn.large_v3_geometry()
    g.enc_layers = g.dec_layers = 2
    spec = syn.model_spec(g, v, n_align=15)
    spec.alignment_heads = [[l, h] for l in range(2) for h in (0, 3, 7, 19)]
    W = syn.random_weights(g, seed=11)
    B, T = 8, 3 + 48
    clips = [syn.synth_audio(400 + i, 480000 - 30000 * i, ("noise", "chirp", "mixed")[i % 3]) for i in range(B)]
    prompt = np.tile(np.array([[v.sot, v.lang_id("en"), v.transcribe]], np.int32), (B, 1))
    runs = []
    engs = [Engine(spec, dtype="bf16", max_batch=B) for _ in range(2)]
    try:
        for e in engs:
            e.load_state_dict(W)
        for rep, e in enumerate([engs[0], engs[0], engs[0], engs[1]]):
            e.mel(clips)
            e.encode(list(range(B)), [0] * B, [3000] * B)
            cap = e.capture_logits(B, T) if rep != 1 else None          # rep 1 goes through the captured hipGraph
            seqs, lens, _ = e.decode(prompt, max_length=T, min_new_tokens=48)
            if cap is not None:
                e.stop_capture()
            runs.append((seqs[:, :T].copy(), None if cap is None else cap[:T - 3].copy(), e.token_timestamps(B, T - 1, 3, [3000] * B)))
        for seqs, cap, ts in runs[1:]:
            assert np.array_equal(seqs, runs[0][0])
            assert np.array_equal(ts, runs[0][2])
            if cap is not None:
                assert np.array_equal(cap, runs[0][1])
    finally:
        for e in engs:
            e.close()


@pytest.mark.parametrize("name", ["beam5_mixed40_b2_n24", "beam3_noise30_b1_n40", "beam2_chirp12_b1_min16", "beam5_noise50_b3_free",
                                  "literal_reference_call_noise20"])
def test_pipeline_beam_search_word_for_word_vs_reference(tiny, name):
    """SURVEY 8(f).4 on the device: items x beams decoder rows, ancestry-indexed self-attention cache, per-row top-k of the
    processed log-probabilities, beam-index gather of the alignment rows -- f32 engine through the drop-in pipeline call
    against transformers run with 2 / 3 / 5 beams, and the LITERAL call of REF/transcribe.py:33 (no generate_kwargs: the
    installed pipeline's 5 beams + language detection): identical text and words, timestamps within one frame."""
    g, v, W, spec = tiny
    meta = Hh.gold_json("e2e_beam_golden.json")[name]
    x = syn.synth_audio(meta["seed"], int(round(meta["secs"] * 16000)), meta["kind"])
    pipe = cw.pipeline("automatic-speech-recognition", model=cw.ModelBundle(spec, W),
                       tokenizer=collate.Vocabulary.from_synthetic(v), chunk_length_s=30,
                       batch_size=meta["batch_size"], return_timestamps="word", torch_dtype="float32", device="cuda:0")
    try:
        out = pipe(x, generate_kwargs=dict(meta["generate_kwargs"])) if meta["generate_kwargs"] else pipe(x)
        assert out["text"] == meta["text"]
        ok, why = Hh.words_equal(out["chunks"], meta["chunks"], tol=0.02)
        assert ok, why
    finally:
        pipe.engine.close()


@pytest.mark.parametrize("dt", ["float32", "bfloat16"])
def test_beam_topk_two_stage_equals_single_block_kernel(tiny, dt):
    """The sliced two-stage candidate selection (16 slices x rows blocks + one merging wave per row) against the single-block
    kernel it replaced, through the whole 5-beam pipeline on 3 chunks (15 rows; prompt step with the begin-suppress /
    max-initial-timestamp rules, text and timestamp phases, forced-timestamp steps): identical words and timestamps."""
    g, v, W, spec = tiny
    x = syn.synth_audio(91, 50 * 16000, "mixed")
    outs = []
    pipe = cw.pipeline("automatic-speech-recognition", model=cw.ModelBundle(spec, W),
                       tokenizer=collate.Vocabulary.from_synthetic(v), chunk_length_s=30, batch_size=3,
                       return_timestamps="word", torch_dtype=dt, device="cuda:0")
    try:
        for one_block in (1, 0):
            assert pipe.engine.lib.cw_test_set_option(b"beam_topk_1block", one_block) == 0
            outs.append(pipe(x, generate_kwargs={**Hh.GEN_KW, "num_beams": 5, "max_new_tokens": 20}))
    finally:
        pipe.engine.lib.cw_test_set_option(b"beam_topk_1block", 0)
        pipe.engine.close()
    assert outs[0]["text"] == outs[1]["text"] and len(outs[0]["chunks"]) > 3
    assert [c["timestamp"] for c in outs[0]["chunks"]] == [c["timestamp"] for c in outs[1]["chunks"]]


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_bench_model_beam_search_16bit_engines(dt):
    """5-beam search with the bench model (large-v3 geometry, aligned synthetic weights) on the 16-bit engines against
    transformers (CPU, fp32, tests/golden/gen_golden_bench_beam.py): 4 bench clips decoded together = 20 decoder rows, 40 tokens
    per pass -- the 17..64-row GEMV path, the shared-K/V cross-attention, the sliced candidate selection and the beam-index gather
    of the alignment rows at full depth.  Every clip must reproduce the reference text with all words within 20 ms."""
    import os
    path = os.path.join(os.path.dirname(__file__), "golden", "e2e_bench_beam_golden.json")
    if not os.path.exists(path):
        pytest.skip("bench-model beam golden not generated")
    gold = Hh.gold_json("e2e_bench_beam_golden.json")
    g, v = syn.large_v3_geometry()
    spec = syn.model_spec(g, v, n_align=15)
    vocab = collate.Vocabulary.from_synthetic(v)
    gk = gold["generate_kwargs"]
    B = len(gold["clips"])
    eng = Engine(spec, dtype=dt, max_batch=B * gk["num_beams"])
    try:
        for n, shape in syn.weight_shapes(g).items():
            eng.load_tensor(n, syn.weight_tensor(g, n, shape, gold["weight_seed"], gold["weights"]))
        clips = [syn.synth_audio(c["seed"], int(c["secs"] * 16000), c["kind"]) for c in gold["clips"]]
        _, nf = eng.mel(clips)
        out = generation.generate(eng, B, nf, language=gk["language"], task=gk["task"], max_new_tokens=gk["max_new_tokens"],
                                  min_new_tokens=gk["min_new_tokens"], num_beams=gk["num_beams"])
        for k, clip in enumerate(gold["clips"]):
            n = len(out["token_timestamps"][k])
            text, words = collate.decode_asr(vocab, [{"tokens": out["sequences"][k][:n], "token_timestamps": out["token_timestamps"][k],
                                                      "stride": (30.0, 0.0, 0.0)}])
            assert text == clip["text"], (clip["seed"], text[:80], clip["text"][:80])
            ok, why = Hh.words_equal(words, clip["chunks"], tol=0.02)
            assert ok, (clip["seed"], why)
    finally:
        eng.close()


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_beam_search_at_the_bench_shape_vs_transformers(dt):
    """What `bench.py --num-beams 5` -- and the literal reference call under transformers 5.x -- decodes: the 8 bench clips x 5
    hypotheses = 40 decoder rows, 128 forced-length tokens per generate call, two seek-loop passes, against transformers (CPU, fp32;
    tests/golden/gen_golden_bench_beam.py with CW_GOLD_CLIPS=8 CW_GOLD_TOKENS=128 -> e2e_bench_beam128_golden.json, round 6).
    f32 engine: every clip word for word.  16-bit engines: beam search ranks hypotheses by cumulative log-probabilities that differ
    by less than the engines' rounding on this synthetic model, so a clip can leave the reference at a near-tie and stay away (there
    is no seam to re-converge at): measured 5 / 8 (bf16) and 6 / 8 (f16) clips identical on the round-5 twelve-launch layer and on the
    round-6 layer (fused stage + column-owning out-projection) alike; asserted: >= 4 clips identical, every word of those within
    20 ms, and a boundary F1 (0.2 s collar) >= 0.9 over all clips.  The 40-token / 20-row golden above stays word for word."""
    import os
    from crisperwhisper_amd import metrics
    path = os.path.join(os.path.dirname(__file__), "golden", "e2e_bench_beam128_golden.json")
    if not os.path.exists(path):
        pytest.skip("bench-shape beam golden not generated")
    gold = Hh.gold_json("e2e_bench_beam128_golden.json")
    g, v = syn.large_v3_geometry()
    spec = syn.model_spec(g, v, n_align=15)
    vocab = collate.Vocabulary.from_synthetic(v)
    gk = gold["generate_kwargs"]
    B = len(gold["clips"])
    eng = Engine(spec, dtype=dt, max_batch=B * gk["num_beams"])
    try:
        for n, shape in syn.weight_shapes(g).items():
            eng.load_tensor(n, syn.weight_tensor(g, n, shape, gold["weight_seed"], gold["weights"]))
        clips = [syn.synth_audio(c["seed"], int(c["secs"] * 16000), c["kind"]) for c in gold["clips"]]
        _, nf = eng.mel(clips)
        out = generation.generate(eng, B, nf, language=gk["language"], task=gk["task"], max_new_tokens=gk["max_new_tokens"],
                                  min_new_tokens=gk["min_new_tokens"], num_beams=gk["num_beams"])
        same, f1s = 0, []
        for k, clip in enumerate(gold["clips"]):
            n = len(out["token_timestamps"][k])
            text, words = collate.decode_asr(vocab, [{"tokens": out["sequences"][k][:n], "token_timestamps": out["token_timestamps"][k],
                                                      "stride": (30.0, 0.0, 0.0)}])
            f1s.append(metrics.boundary_f1(clip["chunks"], words, 0.2)[2])
            if text == clip["text"]:
                ok, why = Hh.words_equal(words, clip["chunks"], tol=0.02)
                assert ok, (clip["seed"], why)
                same += 1
            elif dt == "f32":
                assert False, (clip["seed"], text[:80], clip["text"][:80])
        print(f"beam search at the bench shape, {dt}: {same}/{B} clips identical text (words within 20 ms), boundary F1 {float(np.mean(f1s)):.4f}")
        assert same >= (B if dt == "f32" else 4) and float(np.mean(f1s)) >= 0.9
    finally:
        eng.close()


def test_bench_model_beam_search_over_the_e4m3_cache_rows_kernel_equals_one_row_blocks():
    """5-beam search of the bench model with the opt-in e4m3 cross-attention cache: the hypotheses of an item go through
    attn_cross_mfma8_rows_kernel (one block per (item, head, key split) for all five) -- against the same engine with one block per
    hypothesis row (test option cross_per_row, the round-4 dispatch).  The partial planes are bit-identical per row, so sequences,
    beam scores' order and token timestamps must be EQUAL, not close.  The reference texts of the bf16-cache golden are counted
    but not asserted (the e4m3 cache is accuracy-gated, greedy 8 / 8 + 64 / 64; no beam golden exists for it)."""
    import os
    from crisperwhisper_amd import _native
    path = os.path.join(os.path.dirname(__file__), "golden", "e2e_bench_beam_golden.json")
    if not os.path.exists(path):
        pytest.skip("bench-model beam golden not generated")
    if os.environ.get("CW_CROSS8_VALU") or os.environ.get("CW_CROSS_PER_ROW"):
        pytest.skip("the rows kernel is the matrix-core path of the default process")
    gold = Hh.gold_json("e2e_bench_beam_golden.json")
    g, v = syn.large_v3_geometry()
    spec = syn.model_spec(g, v, n_align=15)
    vocab = collate.Vocabulary.from_synthetic(v)
    gk = gold["generate_kwargs"]
    B = len(gold["clips"])
    lib = _native.load()
    eng = Engine(spec, dtype="bf16", max_batch=B * gk["num_beams"], cross_kv_dtype="fp8")
    outs = {}
    try:
        for n, shape in syn.weight_shapes(g).items():
            eng.load_tensor(n, syn.weight_tensor(g, n, shape, gold["weight_seed"], gold["weights"]))
        clips = [syn.synth_audio(c["seed"], int(c["secs"] * 16000), c["kind"]) for c in gold["clips"]]
        for per_row in (0, 1):
            assert lib.cw_test_set_option(b"cross_per_row", per_row) == 0
            _, nf = eng.mel(clips)
            outs[per_row] = generation.generate(eng, B, nf, language=gk["language"], task=gk["task"], max_new_tokens=gk["max_new_tokens"],
                                                min_new_tokens=gk["min_new_tokens"], num_beams=gk["num_beams"])
    finally:
        lib.cw_test_set_option(b"cross_per_row", 0)
        eng.close()
    a, b = outs[0], outs[1]
    same_text = 0
    for k, clip in enumerate(gold["clips"]):
        assert list(a["sequences"][k]) == list(b["sequences"][k]), (k, a["sequences"][k][:12], b["sequences"][k][:12])
        assert np.array_equal(np.asarray(a["token_timestamps"][k]), np.asarray(b["token_timestamps"][k])), k
        n = len(a["token_timestamps"][k])
        assert n > 8
        text, words = collate.decode_asr(vocab, [{"tokens": a["sequences"][k][:n], "token_timestamps": a["token_timestamps"][k],
                                                  "stride": (30.0, 0.0, 0.0)}])
        assert isinstance(text, str) and len(words) > 0
        same_text += int(text == clip["text"])
    print(f"[e4m3 cache, 5 beams] {same_text} / {B} clips reproduce the bf16-cache reference text")


def test_beam_search_bf16_engine_many_rows_tracks_f32_engine(tiny):
    """bf16 engine, 4 chunks x 5 beams = 20 decoder rows (the 17..64-row GEMV path + ancestry attention + the key-split
    cross-attention shared per item): runs, is well formed, and its first generate call picks the f32 engine's hypotheses
    on most rows (random-weight logits are full of near ties, so this is a sanity bound, not a parity claim)."""
    g, v, W, spec = tiny
    x = syn.synth_audio(77, 70 * 16000, "mixed")
    outs = {}
    for dt in ("float32", "bfloat16"):
        pipe = cw.pipeline("automatic-speech-recognition", model=cw.ModelBundle(spec, W),
                           tokenizer=collate.Vocabulary.from_synthetic(v), chunk_length_s=30, batch_size=4,
                           return_timestamps="word", torch_dtype=dt, device="cuda:0")
        try:
            outs[dt] = pipe(x, generate_kwargs={**Hh.GEN_KW, "num_beams": 5, "max_new_tokens": 12})
        finally:
            pipe.engine.close()
    a, b = outs["float32"], outs["bfloat16"]
    assert isinstance(b["text"], str) and len(b["chunks"]) > 0
    assert "".join(c["text"] for c in b["chunks"]) == b["text"]
    for c in b["chunks"]:
        assert np.isfinite(c["timestamp"][0]) and c["timestamp"][1] >= c["timestamp"][0]
    same = sum(1 for p_, q_ in zip(a["chunks"], b["chunks"]) if p_["text"] == q_["text"])
    assert same >= 0.5 * len(a["chunks"]), (same, len(a["chunks"]))


def _words_close(a_words, b_words, tol=0.02):
    n = ok = 0
    for a, b in zip(a_words, b_words):
        n += 1
        ok += int(a["text"] == b["text"] and all(abs(x - y) <= tol + 1e-9 for x, y in zip(a["timestamp"], b["timestamp"])))
    return ok, n

@pytest.mark.parametrize("dtype", ["bf16", "f16", "bf16+fp8"])
def test_batch64_free_running_every_clip_vs_transformers(dtype):
    """BASELINE configs[3]'s batch in the parity dtypes: 64 x 30 s clips (noise seeds 0..63) decoded together -- the 17..64-row
    decoder path, 128 tokens per pass, free-running through the seek loop -- against the reference pipeline run clip by clip
    through transformers on the CPU in fp32 (tests/golden/gen_golden_bench.py seeds 0..7, gen_golden_bench64.py seeds 8..63).
    Every clip of the batch is compared: identical text, words within 20 ms (measured on MI355X: 64 / 64, 2496 / 2496).
    "bf16+fp8" = the fp8 mode of BASELINE configs[3] that still holds this bar: fc1 of the encoder as an e4m3 MFMA GEMM + the e4m3
    cross-attention cache, the largest e4m3 subset that reproduces all 64 clips (sweep: profiles/r04_fp8_sweep.txt)."""
    import os
    gold = {}
    for name in ("e2e_bench_golden.json", "e2e_bench_b64_golden.json"):
        path = os.path.join(os.path.dirname(__file__), "golden", name)
        if not os.path.exists(path):
            pytest.skip(f"{name} not generated")
        gj = Hh.gold_json(name)
        for c in gj["clips"]:
            gold.setdefault(int(c["seed"]), c)
        gk = gj["generate_kwargs"]
    assert sorted(gold) == list(range(64))
    g, v = syn.large_v3_geometry()
    spec = syn.model_spec(g, v, n_align=15)
    vocab = collate.Vocabulary.from_synthetic(v)
    fp8 = dtype.endswith("+fp8")
    eng = Engine(spec, dtype=dtype.split("+")[0], max_batch=64, cross_kv_dtype="fp8" if fp8 else None)
    try:
        for n, shape in syn.weight_shapes(g).items():
            eng.load_tensor(n, syn.weight_tensor(g, n, shape, 0, "aligned"))
        if fp8:
            eng.check_weights()
            eng.set_encoder_gemm_fp8("fc1")
        _, nf = eng.mel([syn.synth_audio(i, 480000, "noise") for i in range(64)])
        out = generation.generate(eng, 64, nf, language=gk["language"], task=gk["task"], max_new_tokens=gk["max_new_tokens"],
                                  min_new_tokens=gk["min_new_tokens"], num_beams=1)
        same = ok = tot = 0
        differing = []
        for k in range(64):
            n = len(out["token_timestamps"][k])
            text, words = collate.decode_asr(vocab, [{"tokens": out["sequences"][k][:n], "token_timestamps": out["token_timestamps"][k],
                                                      "stride": (30.0, 0.0, 0.0)}])
            if text == gold[k]["text"] and len(words) == len(gold[k]["chunks"]):
                same += 1
                a, b = _words_close(words, gold[k]["chunks"])
                ok += a; tot += b
            else:
                differing.append(k)
        print(f"batch 64 {dtype}: {same}/64 clips identical text, {ok}/{tot} words within 0.02 s, differing {differing}")
        assert same == 64 and ok >= 0.99 * tot and tot > 0, (same, ok, tot, differing)
    finally:
        eng.close()

@pytest.mark.parametrize("B", [16, 17, 33, 48])
def test_odd_batch_sizes_free_running_vs_transformers(B):
    """The decoder's row-count regimes at the bench geometry, free-running bf16 against each clip's transformers reference: 16 rows
    (the reference's own batch_size, REF/transcribe.py:27: last size of the <= 16-row latency path), 17 and 33 (first rows of the
    second and third MFMA row tile of the 17..64-row path: 15 and 31 padded rows), 48 (three full tiles).  Rows are independent, so
    every clip must come out as it does at batch 8 / 64: identical text, words within 20 ms."""
    import os
    gold = {}
    for name in ("e2e_bench_golden.json", "e2e_bench_b64_golden.json"):
        path = os.path.join(os.path.dirname(__file__), "golden", name)
        if not os.path.exists(path):
            pytest.skip(f"{name} not generated")
        gj = Hh.gold_json(name)
        for c in gj["clips"]:
            gold.setdefault(int(c["seed"]), c)
        gk = gj["generate_kwargs"]
    g, v = syn.large_v3_geometry()
    spec = syn.model_spec(g, v, n_align=15)
    vocab = collate.Vocabulary.from_synthetic(v)
    eng = Engine(spec, dtype="bf16", max_batch=B)
    try:
        for n, shape in syn.weight_shapes(g).items():
            eng.load_tensor(n, syn.weight_tensor(g, n, shape, 0, "aligned"))
        _, nf = eng.mel([syn.synth_audio(i, 480000, "noise") for i in range(B)])
        out = generation.generate(eng, B, nf, language=gk["language"], task=gk["task"], max_new_tokens=gk["max_new_tokens"],
                                  min_new_tokens=gk["min_new_tokens"], num_beams=1)
        same = ok = tot = 0
        for k in range(B):
            n = len(out["token_timestamps"][k])
            text, words = collate.decode_asr(vocab, [{"tokens": out["sequences"][k][:n], "token_timestamps": out["token_timestamps"][k],
                                                      "stride": (30.0, 0.0, 0.0)}])
            if text == gold[k]["text"] and len(words) == len(gold[k]["chunks"]):
                same += 1
                a, b = _words_close(words, gold[k]["chunks"])
                ok += a; tot += b
        print(f"batch {B} bf16: {same}/{B} clips identical text, {ok}/{tot} words within 0.02 s")
        assert same == B and ok >= 0.99 * tot and tot > 0, (same, ok, tot)
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_bench_geometry_second_weight_seed_other_audio(dtype):
    """The bench-geometry parity is not tuned to one weight set / one clip family: a second seed of the aligned synthetic
    weights on `mixed` and `chirp` clips (tests/golden/gen_golden_bench2.py seed1: transformers 5.15.0, CPU fp32, 128 tokens per
    generate call), free-running 16-bit engine through the public pipeline call: identical text, words within one frame."""
    import os
    path = os.path.join(os.path.dirname(__file__), "golden", "e2e_bench_seed1_golden.json")
    if not os.path.exists(path):
        pytest.skip("second-seed bench golden not generated")
    gold = Hh.gold_json("e2e_bench_seed1_golden.json")
    g, v = syn.large_v3_geometry()
    spec = syn.model_spec(g, v, n_align=15)
    pipe = cw.pipeline("automatic-speech-recognition", model=cw.ModelBundle(spec, dict(_aligned_weights(g, gold["weight_seed"]).items())),
                       tokenizer=collate.Vocabulary.from_synthetic(v), chunk_length_s=30, batch_size=4, return_timestamps="word",
                       torch_dtype={"bf16": "bfloat16", "f16": "float16"}[dtype], device="cuda:0")
    try:
        same = ok = tot = 0
        for c in gold["clips"]:
            x = syn.synth_audio(c["seed"], 480000, c["kind"])
            if c["kind"] == "chirp":                        # as in the generator: the synthetic chirp is deterministic
                x = (np.roll(x, c["seed"] * 1000) * (1.0 + 0.1 * (c["seed"] % 3))).astype(np.float32)
            out = pipe(x, generate_kwargs=dict(gold["generate_kwargs"]))
            same += int(out["text"] == c["text"] and len(out["chunks"]) == len(c["chunks"]))
            if out["text"] == c["text"]:
                a, b = _words_close(out["chunks"], c["chunks"])
                ok += a; tot += b
        print(f"second seed {dtype}: {same}/{len(gold['clips'])} clips identical text, {ok}/{tot} words within 0.02 s")
        assert same == len(gold["clips"]) and ok >= 0.99 * tot and tot > 0
    finally:
        pipe.engine.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_longform_600s_at_bench_geometry_vs_transformers(dtype):
    """BASELINE configs[2] at full geometry against the reference: the 600 s recording of bench.py's longform leg through
    transformers.pipeline(chunk_length_s=30, batch_size=4) on the CPU (tests/golden/gen_golden_bench2.py longform: 30 chunks, 5 s
    strides, 29 seams merged by _decode_asr) and through the drop-in pipeline with the same arguments.  f32 engine: word for
    word; 16-bit engines (free-running over 30 chunks; f16 is the reference's own GPU dtype, REF/transcribe.py:10): >= 98.5 % of
    the reference words reproduced within one frame (measured, round 6: bf16 1104 of 1113, f16 1113 of 1113 with identical text; gpurun_out/parity_longform_*.json), measured by the longest common word subsequence so
    that a single divergent chunk cannot shift everything after it.  Why not 100 %: profiles/r04_longform_divergence.txt lists
    every decoder row that parts from the reference with the f32 engine's logit margin at that token -- 0.0009-0.039 on a logit
    range of 17, inside the 16-bit engines' own rounding noise (rms 0.011 / 0.003): ties, broken differently."""
    import os, difflib
    path = os.path.join(os.path.dirname(__file__), "golden", "e2e_bench_longform_golden.json")
    if not os.path.exists(path):
        pytest.skip("longform bench golden not generated")
    gold = Hh.gold_json("e2e_bench_longform_golden.json")
    g, v = syn.large_v3_geometry()
    spec = syn.model_spec(g, v, n_align=15)
    a = gold["audio"]
    x = syn.synth_audio(a["seed"], a["secs"] * 16000, a["kind"])
    pipe = cw.pipeline("automatic-speech-recognition", model=cw.ModelBundle(spec, dict(_aligned_weights(g, gold["weight_seed"]).items())),
                       tokenizer=collate.Vocabulary.from_synthetic(v), chunk_length_s=gold["pipeline"]["chunk_length_s"],
                       batch_size=gold["pipeline"]["batch_size"], return_timestamps="word",
                       torch_dtype={"bf16": "bfloat16", "f32": "float32", "f16": "float16"}[dtype], device="cuda:0")
    try:
        out = pipe(x, generate_kwargs=dict(gold["generate_kwargs"]))
        ref = gold["chunks"]
        sm = difflib.SequenceMatcher(a=[w["text"] for w in ref], b=[w["text"] for w in out["chunks"]], autojunk=False)
        matched = close = 0
        for blk in sm.get_matching_blocks():
            for k in range(blk.size):
                matched += 1
                ra, ob = ref[blk.a + k], out["chunks"][blk.b + k]
                close += int(all(abs(p_ - q_) <= 0.02 + 1e-9 for p_, q_ in zip(ra["timestamp"], ob["timestamp"])))
        print(f"longform {dtype}: {len(out['chunks'])} words (reference {len(ref)}), {matched} in common order, {close} of them within 0.02 s, "
              f"identical text: {out['text'] == gold['text']}")
        try:
            import json
            os.makedirs("gpurun_out", exist_ok=True)
            json.dump({"words": len(out["chunks"]), "reference_words": len(ref), "matched": matched, "within_20ms": close,
                       "identical_text": out["text"] == gold["text"]}, open(f"gpurun_out/parity_longform_{dtype}.json", "w"))
        except OSError:
            pass
        if dtype == "f32":
            assert out["text"] == gold["text"]
            ok, why = Hh.words_equal(out["chunks"], ref, tol=0.02)
            assert ok, why
        else:
            assert close >= 0.985 * len(ref), (close, matched, len(ref))
    finally:
        pipe.engine.close()

@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_thresholds_at_bench_geometry_through_the_native_seek_loop(dtype):
    """logprob_threshold / no_speech_threshold at the BENCH geometry (large-v3 shapes, aligned weights) through the public
    pipeline call, i.e. cw_transcribe's own skip logic and the samplers' log-probability tracking at full size, in the parity
    engine and in both 16-bit engines: golden = the reference pipeline call through transformers with thresholds placed between
    the probed values so that one window is skipped (tests/golden/gen_golden_thresholds_bench.py: 100 s recording, 5 chunks, 10
    passes).  Identical text, words within 20 ms, fewer words than without thresholds; the two compared quantities of the first
    window agree with what transformers compared."""
    import os
    path = os.path.join(os.path.dirname(__file__), "golden", "e2e_thresholds_bench_golden.json")
    if not os.path.exists(path):
        pytest.skip("bench-geometry thresholds golden not generated")
    gold = Hh.gold_json("e2e_thresholds_bench_golden.json")
    from tests.golden.gen_golden_thresholds import audio
    x = audio()[: gold["seconds"] * 16000]
    g, v = syn.large_v3_geometry()
    spec = syn.model_spec(g, v, n_align=15)
    pipe = cw.pipeline("automatic-speech-recognition", model=cw.ModelBundle(spec, dict(_aligned_weights(g, gold["weight_seed"]).items())),
                       tokenizer=collate.Vocabulary.from_synthetic(v), chunk_length_s=30, batch_size=gold["batch_size"], return_timestamps="word",
                       torch_dtype={"bf16": "bfloat16", "f16": "float16", "f32": "float32"}[dtype], device="cuda:0", num_beams=1)
    try:
        gk = gold["generate_kwargs"]
        eng = pipe.engine
        _, nf = eng.mel([x[:480000]])
        eng.encode([0], [0], [3000])
        eng.set_thresholds(gk["logprob_threshold"], gk["no_speech_threshold"])
        nsp = eng.no_speech_probs(1, v.sot)
        eng.decode(np.array([[v.sot, v.lang_id("en"), v.transcribe]], np.int32), max_length=3 + gk["max_new_tokens"])
        alp = eng.avg_logprobs(1)
        want = gold["passes"][0][0]
        print(f"thresholds {dtype}: first window avg_logprob {float(alp[0]):.4f} (reference {want['avg_logprob']:.4f}), "
              f"no_speech_prob {float(nsp[0]):.3e} (reference {want['no_speech_prob']:.3e})")
        assert abs(float(alp[0]) - want["avg_logprob"]) <= (2e-3 if dtype == "f32" else 3e-2), (alp, want)
        out = pipe(x, generate_kwargs=dict(gk))
        assert out["text"] == gold["text"]
        ok, why = Hh.words_equal(out["chunks"], gold["chunks"], tol=0.02)
        assert ok, why
        assert len(out["chunks"]) < gold["n_words_without_thresholds"]
    finally:
        pipe.engine.close()


@pytest.mark.parametrize("case", ["greedy"])
def test_logprob_and_no_speech_thresholds_vs_transformers(tiny, case):
    """The deterministic half of generate_with_fallback: with `logprob_threshold` and `no_speech_threshold` set (and
    temperature 0) transformers skips a window whose average token log-probability is low and whose no-speech probability is
    high (generation_whisper.py:879-881, 1243-1287; logits_process.py:2050-2112).  Golden: the reference pipeline call with
    thresholds placed so that some second passes are skipped (tests/golden/gen_golden_thresholds.py).  f32 engine, same call:
    identical text and words; and the two quantities themselves agree with what HF compared."""
    g, v, W, spec = tiny
    gold = Hh.gold_json("e2e_thresholds_golden.json")
    c = gold["cases"][case]
    from tests.golden.gen_golden_thresholds import audio
    x = audio()
    pipe = cw.pipeline("automatic-speech-recognition", model=cw.ModelBundle(spec, W), tokenizer=collate.Vocabulary.from_synthetic(v),
                       chunk_length_s=30, batch_size=gold["batch_size"], return_timestamps="word", torch_dtype="float32",
                       device="cuda:0", num_beams=2)
    try:
        out = pipe(x, generate_kwargs=dict(c["generate_kwargs"]))
        assert out["text"] == c["text"]
        ok, why = Hh.words_equal(out["chunks"], c["chunks"], tol=0.02)
        assert ok, why
        assert len(out["chunks"]) < c["n_words_without_thresholds"]          # something was skipped
        if case == "greedy":
            # the quantities HF compared, for the first window of the recording (first pass of chunk 0)
            eng = pipe.engine
            w0 = x[:480000]
            _, nf = eng.mel([w0])
            eng.encode([0], [0], [3000])
            eng.set_thresholds(c["generate_kwargs"]["logprob_threshold"], c["generate_kwargs"]["no_speech_threshold"])
            nsp = eng.no_speech_probs(1, v.sot)
            prompt = np.array([[v.sot, v.lang_id("en"), v.transcribe]], np.int32)
            eng.decode(prompt, max_length=3 + c["generate_kwargs"]["max_new_tokens"])
            alp = eng.avg_logprobs(1)
            want = c["passes"][0][0]
            assert abs(float(nsp[0]) - want["no_speech_prob"]) <= 1e-4 * max(1.0, want["no_speech_prob"]) + 1e-7, (nsp, want)
            assert abs(float(alp[0]) - want["avg_logprob"]) <= 2e-3, (alp, want)
            # the seek loop inside the library (cw_transcribe) and the stage-by-stage host loop skip the same windows
            from crisperwhisper_amd import generation
            wins = [x[k * 400000: k * 400000 + 480000] for k in range(2)]
            kw = dict(language="<|en|>", task="transcribe", max_new_tokens=c["generate_kwargs"]["max_new_tokens"],
                      logprob_threshold=c["generate_kwargs"]["logprob_threshold"], no_speech_threshold=c["generate_kwargs"]["no_speech_threshold"])
            outs = []
            for native in (True, False):
                _, nf = eng.mel(wins)
                outs.append(generation.generate(eng, 2, nf, native=native, **kw))
            assert outs[0]["sequences"].tolist() == outs[1]["sequences"].tolist()
            for a_, b_ in zip(outs[0]["token_timestamps"], outs[1]["token_timestamps"]):
                assert np.array_equal(a_, b_)
    finally:
        pipe.engine.close()


def test_unknown_generate_kwargs_raise_instead_of_being_dropped(tiny):
    g, v, W, spec = tiny
    pipe = cw.pipeline("automatic-speech-recognition", model=cw.ModelBundle(spec, W), tokenizer=collate.Vocabulary.from_synthetic(v),
                       chunk_length_s=30, batch_size=1, return_timestamps="word", torch_dtype="float32", device="cuda:0")
    x = syn.synth_audio(1, 16000, "noise")
    try:
        for bad in ({"repetition_penalty": 1.2}, {"no_repeat_ngram_size": 3}, {"condition_on_prev_tokens": True}, {"do_sample": True},
                    {"temperature": 0.7}, {"temperature": (0.0, 0.2), "logprob_threshold": -1.0}, {"num_return_sequences": 2},
                    {"no_speech_threshold": 0.6}, {"logprob_threshold": -1.0},
                    {"num_beams": 2, "temperature": 0.0, "logprob_threshold": -1.0, "no_speech_threshold": 0.6}):
            with pytest.raises(ValueError):
                pipe(x, generate_kwargs={**{"num_beams": 1, "language": "<|en|>"}, **bad})
        pipe(x, generate_kwargs={"num_beams": 1, "language": "<|en|>", "task": "transcribe", "max_new_tokens": 4, "temperature": 0.0,
                                 "do_sample": False, "compression_ratio_threshold": 1.35})
    finally:
        pipe.engine.close()

@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("rows", [1, 8, 13])
def test_logits_projection_persistent_column_loop_is_bit_identical(dt, rows):
    """The 51866-column logits projection (final LayerNorm + tied proj_out, TF modeling_whisper.py:790, 1080) as a persistent
    column loop (gemm.hip: gemv_loop_kernel: one resident grid, rows normalised once per block, next tile's weights requested
    under the current tile's MFMAs) against the three-tiles-per-block launch of the same arithmetic: identical bits for every
    logit of every row, 1 / 8 / 13 rows (two and four rows per wave), teacher-forced over several positions."""
    g, v = syn.large_v3_geometry()
    g.enc_layers = g.dec_layers = 2
    spec = syn.model_spec(g, v, n_align=15)
    spec.alignment_heads = [[l, h] for l in range(2) for h in (0, 3, 7, 19)]
    W = syn.random_weights(g, seed=21)
    T = 8
    clips = [syn.synth_audio(700 + i, 480000 - 11000 * i, ("noise", "chirp", "mixed")[i % 3]) for i in range(rows)]
    rng = np.random.default_rng(5)
    ids = np.concatenate([[v.sot, v.lang_id("en"), v.transcribe], [v.timestamp_begin], rng.integers(300, 50000, T - 4)])
    forced = np.full((rows, T), -1, np.int32); forced[:, 3:] = ids[3:]
    prompt = np.tile(ids[None, :3], (rows, 1))
    eng = Engine(spec, dtype=dt, max_batch=rows)
    try:
        eng.load_state_dict(W)
        eng.mel(clips)
        eng.encode(list(range(rows)), [0] * rows, [3000] * rows)
        res = {}
        for loop in (1, 0):
            assert eng.lib.cw_test_set_option(b"gemv_loop", loop) == 0
            cap = eng.capture_logits(rows, T)
            eng.decode(prompt, max_length=T, forced=forced)
            res[loop] = cap[:T - 3].copy()
            eng.stop_capture()
        assert np.isfinite(res[1]).all() and np.abs(res[1]).max() > 0
        assert np.array_equal(res[1], res[0]), int((res[1] != res[0]).sum())
    finally:
        eng.lib.cw_test_set_option(b"gemv_loop", 1)
        eng.close()


@pytest.mark.parametrize("rows,dt", [(64, "bf16"), (40, "bf16"), (33, "f16")])
def test_row_groups_and_tile_pairs_of_the_33_to_64_row_gemvs_are_bit_identical(rows, dt):
    """gemm.hip: gemv_mt_kernel<.., NT> with row groups -- the decode projections of 33..64 rows as blocks of two column tiles x
    two of the (up to four) row tiles (default where that leaves >= 160 blocks), as two row groups of one column tile, and as
    the round-3 block (16 columns x every row tile): rows and column tiles are independent in the MFMA, so every logit of a
    teacher-forced run is bit-identical across the three (TF modeling_whisper.py:448-505, the decoder layer's projections)."""
    g, v = syn.large_v3_geometry()
    g.enc_layers, g.dec_layers = 1, 2
    spec = syn.model_spec(g, v, n_align=10)
    spec.alignment_heads = [[l, h] for l in range(2) for h in (0, 3, 7, 19, 11)]
    W = syn.random_weights(g, seed=29)
    T = 8
    clips = [syn.synth_audio(1200 + i, 480000 - 3000 * i, ("noise", "chirp", "mixed")[i % 3]) for i in range(rows)]
    rng = np.random.default_rng(11)
    ids = np.concatenate([[v.sot, v.lang_id("en"), v.transcribe], [v.timestamp_begin], rng.integers(300, 50000, T - 4)])
    forced = np.full((rows, T), -1, np.int32); forced[:, 3:] = ids[3:]
    prompt = np.tile(ids[None, :3], (rows, 1))
    eng = Engine(spec, dtype=dt, max_batch=rows)
    try:
        eng.load_state_dict(W)
        eng.mel(clips)
        eng.encode(list(range(rows)), [0] * rows, [3000] * rows)
        res = {}
        for var in (-1, 0, 1, 2):
            assert eng.lib.cw_test_set_option(b"mt_variant", var) == 0
            cap = eng.capture_logits(rows, T)
            eng.decode(prompt, max_length=T, forced=forced)
            res[var] = cap[:T - 3].copy()
            eng.stop_capture()
        assert np.isfinite(res[0]).all() and np.abs(res[0]).max() > 0
        for var in (-1, 1, 2):
            assert np.array_equal(res[var], res[0]), (var, int((res[var] != res[0]).sum()))
    finally:
        eng.lib.cw_test_set_option(b"mt_variant", -1)
        eng.close()


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("rows", [2, 5, 8, 11, 16])
def test_combining_out_projection_in_row_groups_is_bit_identical(dt, rows):
    """The cross-attention out-projection of <= 8 rows (gemm.hip: gemv2_bf16_kernel<.., COMBINE>: combines the six key-split
    partials, TF modeling_whisper.py:286-300 + 496-503) as grid (N / 32, K slices, row groups) -- 240 blocks of 87 KB instead
    of 160 of 145 KB -- against the (N / 16, K slices) launch: same K slices, same summation orders, so every logit of a
    teacher-forced run over several positions is bit-identical (graph replay included: decode() without capture follows)."""
    g, v = syn.large_v3_geometry()
    g.enc_layers, g.dec_layers = 1, 3
    spec = syn.model_spec(g, v, n_align=15)
    spec.alignment_heads = [[l, h] for l in range(3) for h in (0, 3, 7, 19, 11)][:15]
    W = syn.random_weights(g, seed=23)
    T = 12
    clips = [syn.synth_audio(900 + i, 480000 - 9000 * i, ("noise", "chirp", "mixed")[i % 3]) for i in range(rows)]
    rng = np.random.default_rng(7)
    ids = np.concatenate([[v.sot, v.lang_id("en"), v.transcribe], [v.timestamp_begin], rng.integers(300, 50000, T - 4)])
    forced = np.full((rows, T), -1, np.int32); forced[:, 3:] = ids[3:]
    prompt = np.tile(ids[None, :3], (rows, 1))
    eng = Engine(spec, dtype=dt, max_batch=rows)
    try:
        eng.load_state_dict(W)
        eng.mel(clips)
        eng.encode(list(range(rows)), [0] * rows, [3000] * rows)
        res = {}
        for on in (1, 0):
            assert eng.lib.cw_test_set_option(b"comb_rowgroups", on) == 0
            cap = eng.capture_logits(rows, T)
            eng.decode(prompt, max_length=T, forced=forced)
            res[on] = (cap[:T - 3].copy(), eng.alignment(rows, T - 1).copy())
            eng.stop_capture()
        assert np.isfinite(res[1][0]).all() and np.abs(res[1][0]).max() > 0
        assert np.array_equal(res[1][0], res[0][0]), int((res[1][0] != res[0][0]).sum())
        assert np.array_equal(res[1][1], res[0][1])
    finally:
        eng.lib.cw_test_set_option(b"comb_rowgroups", -1)
        eng.close()


@pytest.mark.parametrize("feature,rows,dt", [("qkv_self", 8, "bf16"), ("qkv_self", 8, "f16"), ("qkv_self", 5, "bf16"), ("qkv_self", 1, "bf16"),
                                             ("declayer", 8, "bf16"), ("declayer", 8, "f16"), ("declayer", 3, "bf16"),
                                             ("mlp_chain", 8, "bf16"), ("mlp_chain", 8, "f16"), ("mlp_chain", 5, "bf16"), ("mlp_chain", 1, "bf16")])
def test_persistent_decoder_layer_is_bit_identical(request, feature, rows, dt):
    """csrc/declayer.hip: decoder stages that hand their results across CUs INSIDE a launch as 8-byte {tag, value} granules.
    qkv_self: LayerNorm + q/k/v projection + self-attention in one launch (default) against CW_NO_QKV_SELF=1 (two launches);
    declayer: fused out-projection / cross-query stage + cross-attention in one persistent launch (CW_DECLAYER=1, one 1024-thread
    workgroup per CU; measured slower, A/B only) against the two launches; mlp_chain: LayerNorm + fc1 + GELU and fc2 + residual in
    one launch (CW_MLP_CHAIN=1; fc2's blocks take their weights at kernel entry and wait for the fc1 blocks' flags; measured slower,
    A/B only) against the two launches.  Same arithmetic in the same order, so EVERYTHING must
    be bit-identical: the logits of the captured steps, every token of > 2000 consecutive free-running decoder forwards (five
    generate calls of 440 positions -- history longer than the 128 keys of the attention's register path -- through graph replay:
    the granule tags come from a device counter), the alignment rows and the token timestamps.  A missed or stale hand-off changes
    bits here, not words."""
    import os
    if feature in ("declayer", "mlp_chain") and not Hh.has_experiments():
        # measured-slower persistent stage: compiled into -DCW_EXPERIMENTS builds only (profiles/r05_declayer_phases.txt, r05_mlp_chain_phases.txt)
        return Hh.run_in_child(request, Hh.experiments_env(), lambda p: p["feature"] in ("declayer", "mlp_chain"))
    g, v = syn.large_v3_geometry()
    g.enc_layers, g.dec_layers = 1, 4
    spec = syn.model_spec(g, v, n_align=15)
    spec.alignment_heads = [[l, h] for l in range(4) for h in (0, 3, 7, 19)][:15]
    W = syn.random_weights(g, seed=21)
    TGT = g.max_target_positions
    T = TGT - 4
    clips = [syn.synth_audio(700 + i, 480000 - 20000 * i, ("noise", "chirp", "mixed")[i % 3]) for i in range(rows)]
    prompt = np.tile(np.array([[v.sot, v.lang_id("en"), v.transcribe]], np.int32), (rows, 1))
    envs = {"qkv_self": ({}, {"CW_NO_QKV_SELF": "1"}), "declayer": ({"CW_DECLAYER": "1", "CW_NO_QKV_SELF": "1"}, {"CW_NO_QKV_SELF": "1"}),
            "mlp_chain": ({"CW_MLP_CHAIN": "1"}, {})}[feature]
    res = {}
    for mode, env in zip(("fused", "launches"), envs):
        os.environ.update(env)
        try:
            eng = Engine(spec, dtype=dt, max_batch=rows)
        finally:
            for k_ in env:
                os.environ.pop(k_, None)
        try:
            eng.load_state_dict(W)
            out = []
            for call in range(5):
                eng.mel(clips[call % rows:] + clips[:call % rows])
                eng.encode(list(range(rows)), [0] * rows, [3000] * rows)
                cap = eng.capture_logits(rows, 24) if call in (0, 3) else None     # calls 1, 2, 4 replay the captured hipGraph
                seqs, lens, _ = eng.decode(prompt, max_length=T, min_new_tokens=T - 3)
                if cap is not None:
                    eng.stop_capture()
                out.append((seqs[:, :T].copy(), None if cap is None else cap[:24].copy(), eng.alignment(rows, T - 1).copy(),
                            eng.token_timestamps(rows, T - 1, 3, [3000] * rows).copy()))
            res[mode] = out
        finally:
            eng.close()
    steps = 0
    for (sa, ca, aa, ta), (sb, cb, ab, tb) in zip(res["fused"], res["launches"]):
        assert np.array_equal(sa, sb), int((sa != sb).sum())
        if ca is not None:
            assert np.array_equal(ca, cb), float(np.abs(ca - cb).max())
        assert np.array_equal(aa, ab)
        assert np.array_equal(ta, tb)
        steps += sa.shape[1] - 3
    assert steps > 2000


@pytest.mark.parametrize("min_new,fail_pos", [(0, 37), (150, 90), (0, 3), (150, 3)])
def test_lost_handoff_costs_a_step_not_a_call(min_new, fail_pos):
    """A wait inside qkv_self_kernel that gives up (GPU shared with other work: the polling blocks hold every slot) must cost the
    decode call ONE step, not the call: the kernel records 1 + the decoder position of the first forward it spoiled, the host sees
    the word with the one-step lag of its "rows still running" read (or when the queue has drained, while no row may finish yet:
    min_new_tokens > 0), rebuilds the sampler's per-row state from the token ids and resumes at that position on the
    launch-per-stage kernels.  The test hook `handoff_fail_pos` makes the item blocks of layer 0 give up at one position and
    carry on with garbage, exactly what a starved poll leaves behind.  Everything the call returns -- tokens, alignment rows, token
    timestamps -- must equal the undisturbed run bit for bit; cw_handoff_fallbacks counts the switch, cw_handoff_resumes that the
    call did not start over.  fail_pos inside the prompt (3 = the last prompt position): the whole call is repeated instead
    (nothing to resume from), same results."""
    g, v = syn.large_v3_geometry()
    g.enc_layers, g.dec_layers = 1, 3
    spec = syn.model_spec(g, v, n_align=15)
    spec.alignment_heads = [[l, h] for l in range(3) for h in (0, 3, 7, 11, 19)]
    W = syn.random_weights(g, seed=33)
    rows, T = 5, 200
    clips = [syn.synth_audio(900 + i, 480000 - 30000 * i, ("noise", "chirp", "mixed")[i % 3]) for i in range(rows)]
    prompt = np.tile(np.array([[v.sot, v.lang_id("en"), v.transcribe, v.timestamp_begin]], np.int32), (rows, 1))
    res = {}
    for mode in ("clean", "disturbed"):
        eng = Engine(spec, dtype="bf16", max_batch=rows)
        try:
            eng.load_state_dict(W)
            eng.mel(clips)
            eng.encode(list(range(rows)), [0] * rows, [3000] * rows)
            if mode == "disturbed":
                eng._chk(eng.lib.cw_set_option(eng.ctx, b"handoff_fail_pos", fail_pos))
            seqs, lens, _ = eng.decode(prompt, max_length=T, min_new_tokens=min_new)
            L = int(max(lens)) - 1
            res[mode] = (seqs.copy(), np.asarray(lens).copy(), eng.alignment(rows, L).copy(), eng.token_timestamps(rows, L, 4, [3000] * rows).copy(),
                         int(eng.lib.cw_handoff_fallbacks(eng.ctx)), int(eng.lib.cw_handoff_resumes(eng.ctx)))
            if mode == "disturbed":       # the context stays on the launch-per-stage kernels: a second call is undisturbed
                seqs2, lens2, _ = eng.decode(prompt, max_length=T, min_new_tokens=min_new)
                assert np.array_equal(seqs2, seqs) and int(eng.lib.cw_handoff_fallbacks(eng.ctx)) == 1
        finally:
            eng.close()
    (sa, la, aa, ta, fa, ra), (sb, lb, ab, tb, fb, rb) = res["clean"], res["disturbed"]
    assert fa == 0 and ra == 0
    assert fb == 1 and rb == (1 if fail_pos >= 4 else 0), (fb, rb)
    assert np.array_equal(la, lb), (la, lb)
    assert np.array_equal(sa, sb), int((sa != sb).sum())
    assert np.array_equal(aa, ab)
    assert np.array_equal(ta, tb)
    assert int(max(la)) - 1 > fail_pos          # the disturbed position was inside the decoded range


def test_granule_epoch_restart_is_invisible():
    """The granule tag of qkv_self_kernel's hand-offs carries 26 bits of the device's forward counter; granules are never cleared, so
    long before the tag can repeat (2^25 announced forwards) the entry points zero the granule buffers and restart the counter at 1
    (engine.hip: epoch_hygiene).  The test hook `test_epoch_forwards` puts a context just below the threshold: the next decode call
    performs the restart, the one after runs on the restarted counter -- tokens, alignment rows and timestamps of both equal those of
    a fresh context bit for bit, no hand-off gives up."""
    g, v = syn.large_v3_geometry()
    g.enc_layers, g.dec_layers = 1, 3
    spec = syn.model_spec(g, v, n_align=15)
    spec.alignment_heads = [[l, h] for l in range(3) for h in (0, 3, 7, 11, 19)]
    W = syn.random_weights(g, seed=35)
    rows, T = 6, 120
    clips = [syn.synth_audio(950 + i, 480000 - 25000 * i, ("noise", "chirp", "mixed")[i % 3]) for i in range(rows)]
    prompt = np.tile(np.array([[v.sot, v.lang_id("en"), v.transcribe, v.timestamp_begin]], np.int32), (rows, 1))
    eng = Engine(spec, dtype="bf16", max_batch=rows)
    try:
        eng.load_state_dict(W)
        eng.mel(clips)
        eng.encode(list(range(rows)), [0] * rows, [3000] * rows)
        outs = []
        for call in range(3):
            if call == 1:
                eng._chk(eng.lib.cw_set_option(eng.ctx, b"test_epoch_forwards", (1 << 25) - 10))
            seqs, lens, _ = eng.decode(prompt, max_length=T, min_new_tokens=T - 4)
            L = int(max(lens)) - 1
            outs.append((seqs.copy(), eng.alignment(rows, L).copy(), eng.token_timestamps(rows, L, 4, [3000] * rows).copy()))
        assert int(eng.lib.cw_handoff_fallbacks(eng.ctx)) == 0
        for k in (1, 2):
            assert np.array_equal(outs[0][0], outs[k][0]) and np.array_equal(outs[0][1], outs[k][1]) and np.array_equal(outs[0][2], outs[k][2])
    finally:
        eng.close()


@pytest.mark.parametrize("kv", [None, "fp8"])
@pytest.mark.parametrize("rows", [3, 8, 12, 17, 40, 64])
def test_fused_decoder_stage_tracks_eight_launch_layer(rows, kv):
    """csrc/decfuse.hip: the out-projection + cross-query stage applied through the load-time product matrix (7 launches per
    layer) against the same engine with the stage switched off (CW_NO_FUSE6=1, 8 launches), large-v3 shapes on a 2+2-layer stack,
    teacher-forced, 1..16 rows (two or four rows per wave): logits within bf16 rounding of each other, same tokens, alignment
    rows within 2e-2 -- the two differ only in where the 16-bit roundings fall (x before the mean is subtracted, the product
    W'q Wo rounded once).  17 / 40 / 64 rows (round 5): the stage in groups of 16 rows (gemv_stack_kernel's grid y, one statistics
    plane per group) against the twelve-launch layer of the 17..64-row path.  kv = "fp8": the same over the e4m3 cross-attention cache, whose matrix-core kernel
    (attn_cross_mfma8_kernel<.., FUSED>) finishes the fused query like the bf16 kernel does."""
    import os
    g, v = syn.large_v3_geometry()
    g.enc_layers = g.dec_layers = 2
    spec = syn.model_spec(g, v, n_align=15)
    spec.alignment_heads = [[l, h] for l in range(2) for h in (0, 3, 7, 19)]
    W = syn.random_weights(g, seed=9)
    T = 10
    clips = [syn.synth_audio(300 + i, 480000 - 15000 * (i % 12), ("noise", "chirp", "mixed")[i % 3]) for i in range(rows)]
    rng = np.random.default_rng(2)
    ids = np.concatenate([[v.sot, v.lang_id("en"), v.transcribe], [v.timestamp_begin], rng.integers(300, 50000, T - 4)])
    forced = np.full((rows, T), -1, np.int32); forced[:, 3:] = ids[3:]
    prompt = np.tile(ids[None, :3], (rows, 1))
    res = {}
    for mode in ("fused", "eight"):
        if mode == "eight":
            os.environ["CW_NO_FUSE6"] = "1"
        try:
            eng = Engine(spec, dtype="bf16", max_batch=rows, cross_kv_dtype=kv)
        finally:
            os.environ.pop("CW_NO_FUSE6", None)
        try:
            eng.load_state_dict(W)
            eng.mel(clips)
            eng.encode(list(range(rows)), [0] * rows, [3000] * rows)
            cap = eng.capture_logits(rows, T)
            eng.decode(prompt, max_length=T, forced=forced)
            res[mode] = (cap[:T - 3].copy(), eng.alignment(rows, T - 1))
            eng.stop_capture()
        finally:
            eng.close()
    (lf, af), (le, ae) = res["fused"], res["eight"]
    rel = np.abs(lf - le).max() / np.abs(le).max()
    assert rel < 0.03, rel
    assert (lf.argmax(-1) == le.argmax(-1)).mean() > 0.95
    assert np.abs(af - ae).max() < 2e-2

@pytest.mark.parametrize("rows", [20, 40])
def test_row_major_decoder_weights_above_16_rows_track_the_packed_path(rows):
    """gemv_mt_kernel (17..64 decoder rows) reads fragment-major weights only since round 6 (a run-time layout flag cost 1.2-2.2 % per
    step: hipcc unswitched the request loop on it).  A context whose decoder weights stay row-major (CW_NO_WPACK=1; geometries
    pack_decoder_weights does not take) runs those rows as groups of 16 on the <= 16-row kernels, unfused.  Same model, same forced
    tokens, large-v3 shapes on a 2 + 2-layer stack: logits within bf16 rounding of the default path, same argmax, alignment rows within
    2e-2 (the two differ in where the 16-bit roundings fall, exactly like the fused stage against the eight-launch layer)."""
    import os
    g, v = syn.large_v3_geometry()
    g.enc_layers = g.dec_layers = 2
    spec = syn.model_spec(g, v, n_align=15)
    spec.alignment_heads = [[l, h] for l in range(2) for h in (0, 3, 7, 19)]
    W = syn.random_weights(g, seed=9)
    T = 10
    clips = [syn.synth_audio(300 + i, 480000 - 15000 * (i % 12), ("noise", "chirp", "mixed")[i % 3]) for i in range(rows)]
    rng = np.random.default_rng(2)
    ids = np.concatenate([[v.sot, v.lang_id("en"), v.transcribe], [v.timestamp_begin], rng.integers(300, 50000, T - 4)])
    forced = np.full((rows, T), -1, np.int32); forced[:, 3:] = ids[3:]
    prompt = np.tile(ids[None, :3], (rows, 1))
    res = {}
    for mode in ("packed", "row_major"):
        if mode == "row_major":
            os.environ["CW_NO_WPACK"] = "1"
        try:
            eng = Engine(spec, dtype="bf16", max_batch=rows)
        finally:
            os.environ.pop("CW_NO_WPACK", None)
        try:
            eng.load_state_dict(W)
            eng.mel(clips)
            eng.encode(list(range(rows)), [0] * rows, [3000] * rows)
            cap = eng.capture_logits(rows, T)
            eng.decode(prompt, max_length=T, forced=forced)
            res[mode] = (cap[:T - 3].copy(), eng.alignment(rows, T - 1))
            eng.stop_capture()
        finally:
            eng.close()
    (lp, ap), (lr, ar) = res["packed"], res["row_major"]
    assert np.isfinite(lr).all() and np.abs(lr).max() > 0
    rel = np.abs(lp - lr).max() / np.abs(lr).max()
    assert rel < 0.03, rel
    assert (lp.argmax(-1) == lr.argmax(-1)).mean() > 0.95
    assert np.abs(ap - ar).max() < 2e-2


def test_fused_decoder_stage_on_rows_with_a_large_mean():
    """The fused out-projection / cross-query stage multiplies the UN-normalised residual row by W'q and lets the consumer
    apply the LayerNorm (csrc/decfuse.hip).  A row whose mean is far from zero (outlier channels, drifting residual streams:
    here every decoder position carries an offset of 40 against a spread of ~1) must not lose that factor of precision: rows
    with |mean| >= std are rounded as x - mean.  Teacher-forced logits of the bf16 engine against the f32 engine: the fused
    stage is as close as the eight-launch layer (which rounds LN(x)); with the centring switched off (CW_NO_STACK_CENTER=1,
    the round-3 arithmetic) it is several times further away."""
    import os
    g, v = syn.large_v3_geometry()
    g.enc_layers = g.dec_layers = 2
    spec = syn.model_spec(g, v, n_align=15)
    spec.alignment_heads = [[l, h] for l in range(2) for h in (0, 3, 7, 19)]
    W = dict(syn.random_weights(g, seed=9))
    W["model.decoder.embed_positions.weight"] = (W["model.decoder.embed_positions.weight"] + 40.0).astype(np.float32)
    rows, T = 8, 10
    clips = [syn.synth_audio(300 + i, 480000 - 15000 * i, ("noise", "chirp", "mixed")[i % 3]) for i in range(rows)]
    rng = np.random.default_rng(2)
    ids = np.concatenate([[v.sot, v.lang_id("en"), v.transcribe], [v.timestamp_begin], rng.integers(300, 50000, T - 4)])
    forced = np.full((rows, T), -1, np.int32); forced[:, 3:] = ids[3:]
    prompt = np.tile(ids[None, :3], (rows, 1))
    res = {}
    for mode, dt, env in (("f32", "f32", None), ("fused", "bf16", None), ("eight", "bf16", "CW_NO_FUSE6"), ("uncentred", "bf16", "CW_NO_STACK_CENTER")):
        if env:
            os.environ[env] = "1"
        try:
            eng = Engine(spec, dtype=dt, max_batch=rows)
        finally:
            if env:
                os.environ.pop(env, None)
        try:
            eng.load_state_dict(W)
            eng.mel(clips)
            eng.encode(list(range(rows)), [0] * rows, [3000] * rows)
            cap = eng.capture_logits(rows, T)
            eng.decode(prompt, max_length=T, forced=forced)
            res[mode] = cap[:T - 3].copy()
            eng.stop_capture()
        finally:
            eng.close()
    ref = res["f32"]
    err = {m: float(np.sqrt(((res[m] - ref) ** 2).mean()) / np.sqrt((ref ** 2).mean())) for m in ("fused", "eight", "uncentred")}
    assert err["fused"] < 1.3 * err["eight"] + 1e-4, err
    assert err["uncentred"] > 1.5 * err["fused"], err          # the guard is doing something on these rows



@pytest.mark.parametrize("rows", [17, 40, 64])
def test_rows_path_without_preparation_launches_tracks_prepared_path(request, rows):
    """csrc/decfuse.hip gemv_rows_kernel: 17..64 decoder rows (beam search, batch 64) with the LayerNorm applied through its
    linearity on the consumer's output and whole-column residual GEMVs (9 launches per layer) against the same engine with a
    preparation launch in front of every GEMV and K-split atomics (`rows_ln` = 0, 12 launches), large-v3 shapes on a 2+2-layer
    stack, teacher-forced: logits within bf16 rounding of each other, same tokens, alignment rows within 2e-2."""
    if not Hh.has_experiments():                     # A/B kernel variant (measured slower): -DCW_EXPERIMENTS builds
        return Hh.run_in_child(request, Hh.experiments_env(), lambda p: True)
    g, v = syn.large_v3_geometry()
    g.enc_layers = g.dec_layers = 2
    spec = syn.model_spec(g, v, n_align=15)
    spec.alignment_heads = [[l, h] for l in range(2) for h in (0, 3, 7, 19)]
    W = syn.random_weights(g, seed=11)
    T = 9
    clips = [syn.synth_audio(500 + i, 480000 - 5000 * i, ("noise", "chirp", "mixed")[i % 3]) for i in range(rows)]
    rng = np.random.default_rng(3)
    ids = np.concatenate([[v.sot, v.lang_id("en"), v.transcribe], [v.timestamp_begin], rng.integers(300, 50000, T - 4)])
    forced = np.full((rows, T), -1, np.int32); forced[:, 3:] = ids[3:]
    prompt = np.tile(ids[None, :3], (rows, 1))
    eng = Engine(spec, dtype="bf16", max_batch=rows)
    res = {}
    try:
        eng.load_state_dict(W)
        eng.mel(clips)
        eng.encode(list(range(rows)), [0] * rows, [3000] * rows)
        for mode in (1, 0):
            eng._chk(eng.lib.cw_set_option(eng.ctx, b"rows_ln", mode))
            cap = eng.capture_logits(rows, T)
            eng.decode(prompt, max_length=T, forced=forced)
            res[mode] = (cap[:T - 3].copy(), eng.alignment(rows, T - 1))
            eng.stop_capture()
    finally:
        eng.close()
    (ln, an), (lo, ao) = res[1], res[0]
    assert np.isfinite(ln).all()
    rel = np.abs(ln - lo).max() / np.abs(lo).max()
    assert rel < 0.03, rel
    assert (ln.argmax(-1) == lo.argmax(-1)).mean() > 0.95
    assert np.abs(an - ao).max() < 2e-2
    assert rel > 0.0          # the two paths are different kernels: identical logits would mean the switch did nothing


@pytest.mark.parametrize("name", ["mixed450_b16_n24", "noise400_b16_free"])
@pytest.mark.parametrize("dtype", ["float32"])
def test_pipeline_at_the_reference_batch_size_16(tiny, name, dtype):
    """REF/transcribe.py:27 constructs its pipeline with batch_size=16: a recording of 400-450 s (16-22 windows: one full
    batch of 16 and a ragged one) through the same call, against transformers (tests/golden/gen_golden_b16.py) -- batch
    composition changes what the reference computes (double crop of the alignment matrix when all windows of a call have the same
    length, batch shrinking in the seek loop), so batch 16 is pinned separately.  f32 engine: word for word."""
    g, v, W, spec = tiny
    meta = Hh.gold_json("e2e_b16_golden.json")[name]
    x = syn.synth_audio(meta["seed"], int(round(meta["secs"] * 16000)), meta["kind"])
    pipe = cw.pipeline("automatic-speech-recognition", model=cw.ModelBundle(spec, W),
                       tokenizer=collate.Vocabulary.from_synthetic(v), chunk_length_s=30,
                       batch_size=16, return_timestamps="word", torch_dtype=dtype, device="cuda:0", num_beams=1)
    try:
        out = pipe(x, generate_kwargs={**Hh.GEN_KW, **meta["extra"]})
        assert out["text"] == meta["text"]
        ok, why = Hh.words_equal(out["chunks"], meta["chunks"], tol=0.02)
        assert ok, why
    finally:
        pipe.engine.close()
