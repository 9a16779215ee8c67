"""Token entropy of the free-running decode (cw_set_token_entropy; the ENT instantiations of sample_partial_kernel / sample_kernel in
csrc/elementwise.hip) on the device: the kernels' value against float64 on the logits of the very step (bound derived in
tests/token_entropy_refs.py), the special rows of the definition, independence of the written token and of the batch, the NaN
pattern of the token log-probabilities, the captured-graph path, masked rows, the switch leaving every existing output alone, the
native seek loop against the host loop, and the pipeline's word values."""
import numpy as np
import pytest

import crisperwhisper_amd as cw
from crisperwhisper_amd import audio, collate, generation, synthetic as syn
from crisperwhisper_amd.engine import Engine, EngineError
from crisperwhisper_amd.generation import stream_id
from tests import helpers as Hh
from tests import sampler_cases as SC
from tests import token_entropy_refs as R
from tests import token_logprob_refs as RL
from tests.test_gpu_score_vs_transformers import BOUND
from tests.test_gpu_token_logprobs import _clips, _prompt, _random_rows

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "bf16", "f16"]
LONG = {"f32": "float32", "bf16": "bfloat16", "f16": "float16"}
GOLD = Hh.gold_json("token_entropy_golden.json")


def gold_tolerance(c, dt, n):
    """Per position of golden case c: what the engine's entropy may differ from transformers' by.  BOUND[dtype] bounds a
    log-probability, a difference of two logits, so it stands for a logit error of half of it; an error of delta in every logit
    moves H by at most delta * slope + delta^2 * curve (tests/golden/gen_golden_token_entropy.py, computed in float64 from the golden
    logits); the f32 engine adds the derived bound of the kernels' own f32 evaluation."""
    delta = BOUND[LONG[dt]] / 2
    tol = delta * np.asarray(c["slope"][:n]) + delta * delta * np.asarray(c["curve"][:n])
    return tol + np.asarray(c["bound"][:n]) if dt == "f32" else tol


@pytest.fixture(scope="module")
def tiny():
    return Hh.tiny_setup()


@pytest.fixture(scope="module")
def engines(tiny):
    g, v, W, spec = tiny
    out = {}
    for dt in DTYPES:
        e = Engine(spec, dtype=dt, max_batch=64)
        e.load_state_dict(W)
        out[dt] = e
    yield out
    for e in out.values():
        e.close()


@pytest.fixture(scope="module")
def large():
    """The sampler at the vocabulary of large-v3 (51 866 columns, four loads per thread), one layer, no weights needed."""
    g, v = syn.large_v3_geometry()
    g.enc_layers = g.dec_layers = 1
    spec = syn.model_spec(g, v, n_align=1)
    spec.alignment_heads = [[0, 0]]
    eng = Engine(spec, dtype="bf16", max_batch=64)
    yield g, v, spec, eng
    eng.close()


def _hook(eng, logits, ids, temp, seed, streams, forced=None, min_new=0, k=0):
    """The hook; its choice and its log-probability are those of the hook without the entropy, bit for bit."""
    out = eng.test_sample_entropy(logits, ids, 3, k, temp, seed, streams if temp > 0 else None, forced=forced, min_new_tokens=min_new)
    choice, lp, ent = out[:3]
    c0, lp0 = eng.test_sample_logprobs(logits, ids, 3, temp, seed, streams if temp > 0 else None, forced=forced, min_new_tokens=min_new)
    assert choice.tolist() == c0.tolist() and lp.tobytes() == lp0.tobytes()
    if k:
        c1, lp1, ti1, tl1 = eng.test_sample_top_logprobs(logits, ids, 3, k, temp, seed, streams if temp > 0 else None, forced=forced,
                                                         min_new_tokens=min_new)
        assert out[3].tobytes() == ti1.tobytes() and out[4].tobytes() == tl1.tobytes() and lp.tobytes() == lp1.tobytes()
    return ent


@pytest.mark.parametrize("temp", [0.0, 0.6])
@pytest.mark.parametrize("dt", DTYPES)
def test_hook_on_the_sampler_cases(tiny, engines, dt, temp):
    """The 57 crafted and random rows of tests/sampler_cases.py, in launches of up to four rows sharing (t, min_new_tokens)."""
    g, v, W, spec = tiny
    eng = engines[dt]
    cs = SC.cases(v, v.size)
    assert len(cs) == 57
    groups = {}
    for i, (name, ids, lg, mn) in enumerate(cs):
        groups.setdefault((len(ids), mn), []).append(i)
    n = 0
    for (t, mn), idx in groups.items():
        for lo in range(0, len(idx), 4):
            sel = idx[lo:lo + 4]
            lg = np.stack([cs[i][2] for i in sel]); ids = np.stack([cs[i][1] for i in sel])
            ent = _hook(eng, lg, ids, temp, 77 + lo, [stream_id(i, 0, 1) for i in sel], min_new=mn, k=(lo // 4) % 2 * 3)
            R.check_rows(ent, lg, spec.vocab_size, what=f"{dt} T={temp} " + ",".join(cs[i][0] for i in sel))
            n += len(sel)
    assert n == 57


def _special_rows(rng, nb, V):
    """(name, logits [nb][V], check) for the rows the definition singles out."""
    out = []
    out.append(("all_equal", np.full((nb, V), -2.5, np.float32)))
    lg = np.full((nb, V), -np.inf, np.float32); lg[np.arange(nb), rng.integers(0, V, nb)] = 7.0
    out.append(("single_finite", lg))
    lg = (rng.standard_normal((nb, V)) * 3).astype(np.float32); lg[np.arange(nb), rng.integers(0, V, nb)] = np.nan
    out.append(("one_nan", lg))
    lg = np.full((nb, V), -np.inf, np.float32); lg[:, V - 1] = np.nan                    # a NaN where no finite logit is met at all
    out.append(("nan_among_minus_inf", lg))
    lg = (rng.standard_normal((nb, V)) * 3).astype(np.float32); lg[:, 5] = np.inf
    out.append(("plus_inf", lg))
    return out


def _rows_checks(eng, v, spec, nb, temp, rng, A, what):
    V = spec.vocab_size
    hist = [spec.timestamp_begin + 3, A]
    ids = np.tile(np.array([v.sot, v.lang_id("en"), v.transcribe] + hist, np.int32), (nb, 1))
    streams = [stream_id(b, 10 * b, 2) for b in range(nb)]
    for name, h, lg, forced in _random_rows(rng, nb, V, spec.timestamp_begin, spec.eos_token_id, A):
        ids_c = np.tile(np.array([v.sot, v.lang_id("en"), v.transcribe] + h, np.int32), (nb, 1))
        ent = _hook(eng, lg, ids_c, temp, 5 + nb, streams, forced=forced, k=4 if name == "spread" else 0)
        R.check_rows(ent, lg, V, what=f"{what} nb={nb} T={temp} {name}")
        if forced is not None:                                   # H does not depend on the token that was written
            ent2 = _hook(eng, lg, ids_c, temp, 5 + nb, streams, forced=None)
            assert ent2.tobytes() == ent.tobytes()
    for name, lg in _special_rows(rng, nb, V):
        ent = _hook(eng, lg, ids, temp, 6 + nb, streams)
        if name == "all_equal":
            R.check_rows(ent, lg, V, what=f"{what} nb={nb} {name}")
            assert np.all(np.abs(ent.astype(np.float64) - np.log(V)) <= [R.bound(lg[b], V) for b in range(nb)])
        elif name == "single_finite":
            assert np.all(ent == 0.0), ent
        else:
            assert np.all(np.isnan(ent)), (name, ent)


@pytest.mark.parametrize("temp", [0.0, 0.6])
@pytest.mark.parametrize("nb", [1, 8, 64])
@pytest.mark.parametrize("dt", DTYPES)
def test_hook_on_random_and_special_rows_tiny_vocabulary(tiny, engines, dt, nb, temp):
    g, v, W, spec = tiny
    _rows_checks(engines[dt], v, spec, nb, temp, np.random.default_rng(1000 * nb + int(temp * 10)), ord("a"), dt)


@pytest.mark.parametrize("temp", [0.0, 0.6])
@pytest.mark.parametrize("nb", [1, 8, 64])
def test_hook_on_random_and_special_rows_large_vocabulary(large, nb, temp):
    g, v, spec, eng = large
    V = spec.vocab_size
    assert V == 51866 and V % 4 and RL.n_iter(V) == 4
    _rows_checks(eng, v, spec, nb, temp, np.random.default_rng(2000 * nb + int(temp * 10)), 300, f"V={V}")


def test_a_rows_bits_do_not_depend_on_the_batch(large):
    """Row b of a 64-row launch and the same row launched alone: the same bits (no atomics, a fixed merge order)."""
    g, v, spec, eng = large
    V = spec.vocab_size
    rng = np.random.default_rng(5)
    lg = rng.uniform(-30, 30, (64, V)).astype(np.float32)
    ids = np.tile(np.array([v.sot, v.lang_id("en"), v.transcribe, spec.timestamp_begin + 3, 300], np.int32), (64, 1))
    full = eng.test_sample_entropy(lg, ids, 3)[2]
    again = eng.test_sample_entropy(lg, ids, 3)[2]
    assert full.tobytes() == again.tobytes()
    for b in (0, 17, 63):
        alone = eng.test_sample_entropy(lg[b:b + 1], ids[b:b + 1], 3)[2]
        assert alone.tobytes() == full[b:b + 1].tobytes()
    perm = rng.permutation(64)
    shuffled = eng.test_sample_entropy(lg[perm], ids, 3)[2]
    assert shuffled.tobytes() == full[perm].tobytes()


def _decode(eng, v, nb, steps, temp, forced=None, capture=False, row_active=None):
    if temp > 0:
        eng.set_sampling(temp, 4242 + nb, [stream_id(b, 0, 3) for b in range(nb)])
    cap = eng.capture_logits(nb, steps) if capture else None
    try:
        seqs, lens, _ = eng.decode(_prompt(v, nb), max_length=3 + steps, forced=forced, row_active=row_active)
        cap = cap.copy() if capture else None
    finally:
        if capture:
            eng.stop_capture()
        eng.set_sampling(0.0)
    return seqs, lens, cap, eng.token_logprobs(nb), eng.token_entropy(nb)


@pytest.mark.parametrize("temp", [0.0, 0.6])
@pytest.mark.parametrize("nb", [1, 8, 9, 17])
@pytest.mark.parametrize("dt", DTYPES)
def test_real_decode_against_float64_on_the_captured_logits(tiny, engines, dt, nb, temp):
    """Free-running, and with an eos forced at a different position per row: every generated position within the bound of float64
    on the logits of its own step, NaN exactly where the token log-probabilities are NaN, the same value whether the position was
    forced or not; the same decode through the captured step graph gives the same bits."""
    g, v, W, spec = tiny
    eng = engines[dt]
    steps, V, tgt = 10, spec.vocab_size, spec.max_target_positions
    eng.mel(_clips(nb))
    eng.encode(list(range(nb)), [0] * nb, [3000] * nb)
    eng.set_token_logprobs(True)
    eng.set_token_entropy(True)
    try:
        forced = np.full((nb, 3 + steps), -1, np.int32)
        for b in range(nb):
            forced[b, 3 + 2 + b % 6] = spec.eos_token_id
        for fr in (None, forced):
            seqs, lens, cap, lp, ent = _decode(eng, v, nb, steps, temp, forced=fr, capture=True)
            assert ent.shape == (nb, tgt) and ent.dtype == np.float32
            assert np.array_equal(np.isnan(ent), np.isnan(lp))
            n = 0
            for b in range(nb):
                L = int(lens[b])
                assert np.all(np.isnan(ent[b, :3])) and np.all(np.isnan(ent[b, L:])) and not np.any(np.isnan(ent[b, 3:L]))
                R.check_rows(ent[b, 3:L], cap[:L - 3, b], V, what=f"{dt} nb={nb} T={temp} forced={fr is not None} row {b}")
                n += L - 3
            assert n >= nb
            seqs2, lens2, _, lp2, ent2 = _decode(eng, v, nb, steps, temp, forced=fr, capture=False)     # captured step graph
            assert seqs2.tobytes() == seqs.tobytes() and lens2.tobytes() == lens.tobytes()
            assert lp2.tobytes() == lp.tobytes() and ent2.tobytes() == ent.tobytes()
    finally:
        eng.set_token_logprobs(False)
    with pytest.raises(EngineError, match="token entropy is off"):
        eng.token_entropy(nb)                           # switching the log-probabilities off switched the entropy off
    with pytest.raises(EngineError, match="needs token log-probabilities"):
        eng.set_token_entropy(True)                     # ... and it cannot come back without them


def test_a_masked_row_keeps_the_values_of_the_decode_before(tiny, engines):
    g, v, W, spec = tiny
    eng = engines["f32"]
    nb, steps = 4, 12
    eng.mel(_clips(nb))
    eng.encode(list(range(nb)), [0] * nb, [3000] * nb)
    eng.set_token_logprobs(True)
    eng.set_token_entropy(True)
    try:
        s0, l0, _, lp0, en0 = _decode(eng, v, nb, steps, 0.0)
        mask = np.array([1, 0, 1, 0], np.int32)
        s1, l1, _, lp1, en1 = _decode(eng, v, nb, steps - 4, 0.8, row_active=mask)
        for b in (1, 3):
            assert en1[b].tobytes() == en0[b].tobytes() and not np.all(np.isnan(en0[b]))
        for b in (0, 2):
            L = int(l1[b])
            assert np.all(np.isnan(en1[b, :3])) and np.all(np.isnan(en1[b, L:])) and not np.any(np.isnan(en1[b, 3:L]))
        assert np.array_equal(np.isnan(en1), np.isnan(lp1))
        assert np.all(np.isnan(eng.token_entropy(8)[nb:]))     # rows never decoded under the switch are NaN
    finally:
        eng.set_token_logprobs(False)


@pytest.mark.parametrize("dt", DTYPES)
def test_the_switch_changes_no_existing_output(tiny, dt):
    g, v, W, spec = tiny
    eng = Engine(spec, dtype=dt, max_batch=8)
    try:
        eng.load_state_dict(W)
        nb = 6
        _, nf = eng.mel(_clips(nb))
        eng.encode(list(range(nb)), [0] * nb, [3000] * nb)
        eng.set_thresholds(-1.0, None)
        eng.set_token_logprobs(True)
        eng.set_top_logprobs(3)
        eng.set_alignment_scores(True)

        def run(temp):
            if temp > 0:
                eng.set_sampling(temp, 3, [stream_id(b, 0, 2) for b in range(nb)])
            try:
                seqs, lens, _ = eng.decode(_prompt(v, nb), max_length=3 + 20)
            finally:
                eng.set_sampling(0.0)
            L = int(lens.max()) - 1
            ts = eng.token_timestamps(nb, L, 3, nf).copy()
            mass, spread = eng.alignment_scores(nb, L)
            ti, tl = eng.top_logprobs(nb)
            return (seqs.copy(), lens.copy(), eng.avg_logprobs(nb).copy(), ts, eng.token_logprobs(nb), ti, tl,
                    np.asarray(mass).copy(), np.asarray(spread).copy(), eng.alignment(nb, L).copy())

        for temp in (0.0, 0.6):
            off = run(temp)
            eng.set_token_entropy(True)
            on = run(temp)
            assert not np.all(np.isnan(eng.token_entropy(nb)))
            eng.set_token_entropy(False)
            off2 = run(temp)
            for a, b, c in zip(off, on, off2):
                assert a.tobytes() == b.tobytes() == c.tobytes()
    finally:
        eng.close()


@pytest.mark.parametrize("prompted", [False, True])
def test_native_seek_loop_equals_host_loop(tiny, engines, prompted):
    g, v, W, spec = tiny
    eng = engines["f32"]
    clips = [syn.synth_audio(60 + i, n, kind) for i, (n, kind) in
             enumerate([(480000, "mixed"), (130000, "noise"), (300001, "chirp"), (1600, "noise")])]
    _, nf = eng.mel(clips)
    sa, sb = {}, {}
    kw = dict(language="<|en|>", task="transcribe", max_new_tokens=40, return_token_logprobs=True)
    if prompted:
        kw["prompt_ids"] = np.array([v.startofprev, ord("h"), ord("i")], np.int64)
    a = generation.generate(eng, len(clips), nf, stats=sa, native=True, return_token_entropy=True, **kw)
    b = generation.generate(eng, len(clips), nf, stats=sb, native=False, return_token_entropy=True, **kw)
    plain = generation.generate(eng, len(clips), nf, native=True, **kw)
    assert sa == sb and sa["generate_calls"] > 1                      # a multi-pass clip
    assert "token_entropy" not in plain and np.array_equal(plain["sequences"], a["sequences"])
    assert np.array_equal(a["sequences"], b["sequences"])
    for x, y, lx, lp_, tx in zip(a["token_entropy"], b["token_entropy"], a["token_logprobs"], plain["token_logprobs"],
                                 a["token_timestamps"]):
        assert x.dtype == np.float32 and y.dtype == np.float32 and len(x) == len(tx) == len(y)
        assert x.tobytes() == y.tobytes() and lx.tobytes() == lp_.tobytes()
        assert not np.any(np.isnan(x)) and np.all(x >= 0) and np.all(x <= np.log(spec.vocab_size) + 1e-4)
    for segs, en in zip(b["segments"], b["token_entropy"]):
        assert sum(len(s.token_entropy) for s in segs) == len(en)
    with pytest.raises(ValueError, match="num_beams"):
        generation.generate(eng, len(clips), nf, num_beams=5, return_token_entropy=True, **{k: x for k, x in kw.items() if k != "prompt_ids"})
    with pytest.raises(ValueError, match="return_token_logprobs"):
        generation.generate(eng, len(clips), nf, language="<|en|>", task="transcribe", return_token_entropy=True)


def _gold_clip(c):
    return syn.synth_audio(c["clip"]["seed"], int(round(c["clip"]["secs"] * 16000)), c["clip"]["kind"])


@pytest.mark.parametrize("dt", DTYPES)
def test_against_transformers(tiny, engines, dt):
    """transformers' greedy sequences and the entropy of the raw logits of each of their steps (generate(output_logits=True),
    tests/golden/gen_golden_token_entropy.py).  f32: the free-running greedy decode produces those tokens word for word; 16-bit
    engines: teacher-forced through cw_decode(forced=...), the same quantity on the same model.  Tolerance: gold_tolerance."""
    g, v, W, spec = tiny
    eng = engines[dt]
    assert GOLD["init"] == [v.sot, v.lang_id("en"), v.transcribe] and GOLD["eos"] == v.eos and GOLD["vocab"] == spec.vocab_size
    worst = 0.0
    for c in GOLD["cases"]:
        ids, ref = np.asarray(c["ids"], np.int64), np.asarray(c["entropy"], np.float64)[:len(c["ids"])]
        _, nf = eng.mel([_gold_clip(c)])
        if dt == "f32":
            out = generation.generate(eng, 1, nf, language="<|en|>", task="transcribe", max_new_tokens=c["max_new_tokens"],
                                      num_beams=1, return_token_logprobs=True, return_token_entropy=True)
            assert out["sequences"][0].tolist() == ids.tolist(), c["clip"]
            got = out["token_entropy"][0]
        else:
            eng.encode([0], [0], [3000])
            forced = np.full((1, 3 + len(ids)), -1, np.int32)
            forced[0, 3:] = ids
            eng.set_token_logprobs(True)
            eng.set_token_entropy(True)
            try:
                seqs, lens, _ = eng.decode(_prompt(v, 1), max_length=3 + len(ids), forced=forced)
                got = eng.token_entropy(1)[0, 3:3 + len(ids)]
            finally:
                eng.set_token_logprobs(False)
            assert seqs[0, 3:3 + len(ids)].tolist() == ids.tolist()
        tol = gold_tolerance(c, dt, len(ids))
        d = np.abs(np.asarray(got, np.float64) - ref)
        print(dt, c["clip"]["seed"], "max |H - ref| =", float(d.max()), "tolerance", float(tol.min()), "..", float(tol.max()))
        worst = max(worst, float((d / tol).max()))
        assert len(got) == len(ref) and np.all(d <= tol), (dt, c["clip"], d.tolist(), tol.tolist())
    print(dt, "worst |H - ref| / tolerance", worst)


@pytest.mark.parametrize("call", ["greedy", "prompt", "fallback", "top"])
def test_pipeline_word_entropy(tiny, call, monkeypatch):
    """A 70 s clip with strides at batch 2: every word carries "entropy" = the float64 mean and "entropy_max" = the maximum of
    generate's token values over the collator's groups; text, timestamps and logprobs are those of the call without it."""
    g, v, W, spec = tiny
    x = syn.synth_audio(0, 70 * 16000, "mixed")
    gk = {"language": "<|en|>", "task": "transcribe", "max_new_tokens": 16, "num_beams": 1}
    extra = {}
    if call == "prompt":
        gk["prompt_ids"] = np.array([v.startofprev, ord("h"), ord("i")], np.int64)
    elif call == "fallback":
        gk.update(temperature=(0.0, 0.6), compression_ratio_threshold=1.2, logprob_threshold=-1.0)
    elif call == "top":
        extra["top_logprobs"] = 2
    pipe = cw.pipeline("automatic-speech-recognition", model=cw.ModelBundle(spec, W), tokenizer=collate.Vocabulary.from_synthetic(v),
                       chunk_length_s=30, batch_size=2, return_timestamps="word", torch_dtype="float32", device="cuda:0",
                       sampling_seed=11)
    try:
        plain = pipe(x, generate_kwargs=dict(gk), return_scores=True, **extra)
        assert all("entropy" not in w for w in plain["chunks"])
        recorded = []
        orig = generation.generate

        def spy(*a, **k):
            out = orig(*a, **k)
            recorded.append((list(k["item_ids"]), out))
            return out

        monkeypatch.setattr(generation, "generate", spy)
        got = pipe(x, generate_kwargs=dict(gk), return_scores=True, return_entropy=True, **extra)
        monkeypatch.undo()
        assert got["text"] == plain["text"] and len(got["chunks"]) > 3
        strip = lambda w: {k: ([{kk: vv for kk, vv in t.items() if kk != "entropy"} for t in val] if k == "tokens" else val)
                           for k, val in w.items() if k not in ("entropy", "entropy_max")}
        assert [strip(w) for w in got["chunks"]] == plain["chunks"]
        windows = audio.chunk_windows(len(x), 480000, 80000, 80000)
        outputs, ens = {}, {}
        for idxs, out in recorded:
            for k, i in enumerate(idxs):
                n = len(out["token_timestamps"][k])
                assert len(out["token_entropy"][k]) == n and out["token_entropy"][k].dtype == np.float32
                outputs[i] = {"tokens": out["sequences"][k][:n], "token_timestamps": out["token_timestamps"][k],
                              "stride": tuple(t / 16000 for t in windows[i][2])}
                ens[i] = out["token_entropy"][k]
        order = sorted(outputs)
        text, words, groups = collate.decode_asr(pipe.vocab, [dict(outputs[i]) for i in order], return_timestamps="word",
                                                 return_token_groups=True)
        flat = np.concatenate([ens[i] for i in order]).astype(np.float64)
        assert text == got["text"] and len(words) == len(got["chunks"])
        for w, grp in zip(got["chunks"], groups):
            assert np.isfinite(w["entropy"]) and 0 <= w["entropy"] <= w["entropy_max"] <= np.log(spec.vocab_size) + 1e-4
            assert w["entropy"] == float(np.mean(flat[grp])) and w["entropy_max"] == float(np.max(flat[grp]))
            if call == "top":
                assert [t["entropy"] for t in w["tokens"]] == [float(flat[i]) for i in grp]
        if call == "fallback":
            assert any(r["temperature_index"] > 0 for r in pipe.stats["fallback"])
        with pytest.raises(ValueError, match="return_entropy"):
            pipe(x, generate_kwargs=dict(gk), return_entropy=True)                       # no return_scores
        with pytest.raises(ValueError, match="beams"):
            pipe(x, generate_kwargs={**gk, "num_beams": 5}, return_scores=True, return_entropy=True)
    finally:
        pipe.engine.close()
