"""Per-token log-probabilities of the free-running decode (cw_set_token_logprobs; sample_partial_kernel / sample_kernel in
csrc/elementwise.hip) on the device: the kernels' value against float64 on the logits of the very step (bound derived in
tests/token_logprob_refs.py), the NaN pattern, the captured-graph path, masked rows, the switch leaving every existing output
alone, the native seek loop against the host loop, transformers' own numbers, and the pipeline's word sums."""
import numpy as np
import pytest

import crisperwhisper_amd as cw
from crisperwhisper_amd import audio, collate, generation, synthetic as syn
from crisperwhisper_amd.engine import Engine
from crisperwhisper_amd.generation import stream_id
from tests import helpers as Hh
from tests import sampler_cases as SC
from tests import token_logprob_refs as R
from tests.test_gpu_score_vs_transformers import BOUND

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "bf16", "f16"]
LONG = {"f32": "float32", "bf16": "bfloat16", "f16": "float16"}
GOLD = Hh.gold_json("token_logprobs_golden.json")


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


def _prompt(v, nb):
    return np.tile(np.array([[v.sot, v.lang_id("en"), v.transcribe]], np.int32), (nb, 1))


def _clips(nb, secs=2):
    kinds = ("noise", "chirp", "mixed")
    return [syn.synth_audio(100 + b, secs * 16000, kinds[b % 3]) for b in range(nb)]


def _hook(eng, logits, ids, temp, seed, streams, forced=None, min_new=0):
    """The hook, its choice held against the existing hooks', the token it wrote and the value it stored for it."""
    choice, lp = eng.test_sample_logprobs(logits, ids, 3, temp, seed, streams if temp > 0 else None, forced=forced,
                                          min_new_tokens=min_new)
    if temp > 0:
        want = eng.test_sample_seeded(logits, ids, 3, temp, seed, streams, min_new_tokens=min_new)
    else:
        want = eng.test_sample(logits, ids, 3, min_new_tokens=min_new)
    assert choice.tolist() == want.tolist()
    tok = choice.copy() if forced is None else np.where(np.asarray(forced) >= 0, forced, choice)
    return tok, lp


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
            tok, lp = _hook(eng, lg, ids, temp, 77 + lo, [stream_id(i, 0, 1) for i in sel], min_new=mn)
            R.check_rows(lp, lg, tok, spec.vocab_size, what=f"{dt} T={temp} " + ",".join(cs[i][0] for i in sel))
            n += len(sel)
    assert n == 57


def _random_rows(rng, nb, V, tb, eos, A):
    """(history, logits [nb][V], forced or None): spread over +-60, a dominant last id next to the pad columns, everything but eos
    masked, a forced token far from the arg-max."""
    out = []
    lg = rng.uniform(-60, 60, (nb, V)).astype(np.float32)
    out.append(("spread", [tb + 3, A], lg, None))
    lg = (rng.standard_normal((nb, V)) * 3).astype(np.float32); lg[:, V - 1] = 35.0
    out.append(("dominant_last_id", [tb + 3, A], lg, None))
    out.append(("dominant_last_id_forced", [tb + 3, A], lg, np.full(nb, V - 1, np.int32)))
    lg = (rng.standard_normal((nb, V)) * 3).astype(np.float32); lg[:, eos + 1:] = -np.inf; lg[:, A] = 20.0
    out.append(("all_but_eos_masked", [tb, A, tb + 10], lg, None))       # after (text, timestamp): nothing below eos is allowed
    lg = (rng.standard_normal((nb, V)) * 3).astype(np.float32); lg[:, A] = 25.0
    forced = rng.integers(A + 1, eos, nb).astype(np.int32); forced[::3] = -1
    out.append(("forced_far_from_argmax", [tb + 3, A], lg, forced))
    return out


@pytest.mark.parametrize("temp", [0.0, 0.6])
@pytest.mark.parametrize("nb", [1, 8, 64])
@pytest.mark.parametrize("dt", DTYPES)
def test_hook_on_random_rows_tiny_vocabulary(tiny, engines, dt, nb, temp):
    g, v, W, spec = tiny
    eng = engines[dt]
    rng = np.random.default_rng(1000 * nb + int(temp * 10))
    for name, hist, lg, forced in _random_rows(rng, nb, spec.vocab_size, spec.timestamp_begin, spec.eos_token_id, ord("a")):
        ids = np.tile(np.array([v.sot, v.lang_id("en"), v.transcribe] + hist, np.int32), (nb, 1))
        tok, lp = _hook(eng, lg, ids, temp, 5 + nb, [stream_id(b, 10 * b, 2) for b in range(nb)], forced=forced)
        if name == "all_but_eos_masked":
            assert np.all(tok == spec.eos_token_id)
        R.check_rows(lp, lg, tok, spec.vocab_size, what=f"{dt} nb={nb} T={temp} {name}")


@pytest.mark.parametrize("temp", [0.0, 0.6])
@pytest.mark.parametrize("nb", [1, 8, 64])
def test_hook_on_random_rows_large_vocabulary(large, nb, temp):
    g, v, spec, eng = large
    V = spec.vocab_size
    assert V == 51866 and V % 4 and R.n_iter(V) == 4
    rng = np.random.default_rng(2000 * nb + int(temp * 10))
    for name, hist, lg, forced in _random_rows(rng, nb, V, spec.timestamp_begin, spec.eos_token_id, 300):
        ids = np.tile(np.array([v.sot, v.lang_id("en"), v.transcribe] + hist, np.int32), (nb, 1))
        tok, lp = _hook(eng, lg, ids, temp, 9 + nb, [stream_id(b, 10 * b, 2) for b in range(nb)], forced=forced)
        if name == "all_but_eos_masked":
            assert np.all(tok == spec.eos_token_id)
        R.check_rows(lp, lg, tok, V, what=f"V={V} nb={nb} T={temp} {name}")


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
    return seqs, lens, cap, eng.token_logprobs(nb)


@pytest.mark.parametrize("temp", [0.0, 0.6])
@pytest.mark.parametrize("nb", [1, 8, 17])
@pytest.mark.parametrize("dt", DTYPES)
def test_real_decode_against_float64_on_the_captured_logits(tiny, engines, dt, nb, temp):
    """Free-running, and with an eos forced at a different position per row so that rows end inside the decode: every generated
    position (the eos included) within the bound of float64 on the logits of its own step, NaN exactly at prompt positions and
    behind each row's end; the same decode through the captured step graph gives the same bits."""
    g, v, W, spec = tiny
    eng = engines[dt]
    steps, V, tgt = 10, spec.vocab_size, spec.max_target_positions
    eng.mel(_clips(nb))
    eng.encode(list(range(nb)), [0] * nb, [3000] * nb)
    eng.set_token_logprobs(True)
    try:
        forced = np.full((nb, 3 + steps), -1, np.int32)
        for b in range(nb):
            forced[b, 3 + 2 + b % 6] = spec.eos_token_id
        for fr in (None, forced):
            seqs, lens, cap, lp = _decode(eng, v, nb, steps, temp, forced=fr, capture=True)
            assert lp.shape == (nb, tgt) and lp.dtype == np.float32
            if fr is not None:                          # the forced eos ends the row, unless it ended by itself before
                assert all(int(lens[b]) <= 3 + 2 + b % 6 + 1 for b in range(nb)) and int(lens[0]) < 3 + steps
            n = 0
            for b in range(nb):
                L = int(lens[b])
                assert np.all(np.isnan(lp[b, :3])) and np.all(np.isnan(lp[b, L:])) and not np.any(np.isnan(lp[b, 3:L]))
                toks = seqs[b, 3:L]
                R.check_rows(lp[b, 3:L], cap[:L - 3, b], toks, V, what=f"{dt} nb={nb} T={temp} forced={fr is not None} row {b}")
                n += L - 3
            assert n >= nb
            seqs2, lens2, _, lp2 = _decode(eng, v, nb, steps, temp, forced=fr, capture=False)     # captured step graph
            assert seqs2.tobytes() == seqs.tobytes() and lens2.tobytes() == lens.tobytes()
            assert lp2.tobytes() == lp.tobytes()
    finally:
        eng.set_token_logprobs(False)


def test_a_masked_row_keeps_the_values_of_the_decode_before(tiny, engines):
    g, v, W, spec = tiny
    eng = engines["f32"]
    nb, steps = 4, 12
    eng.mel(_clips(nb))
    eng.encode(list(range(nb)), [0] * nb, [3000] * nb)
    eng.set_token_logprobs(True)
    try:
        s0, l0, _, lp0 = _decode(eng, v, nb, steps, 0.0)
        mask = np.array([1, 0, 1, 0], np.int32)
        s1, l1, _, lp1 = _decode(eng, v, nb, steps - 4, 0.8, row_active=mask)
        assert l1[1] == 0 and l1[3] == 0
        for b in (1, 3):
            assert lp1[b].tobytes() == lp0[b].tobytes()
        for b in (0, 2):
            L = int(l1[b])
            assert s1[b, :L].tolist() != s0[b, :L].tolist() or L != int(l0[b])
            assert np.all(np.isnan(lp1[b, :3])) and np.all(np.isnan(lp1[b, L:])) and not np.any(np.isnan(lp1[b, 3:L]))
        # rows never decoded under the switch are NaN
        assert np.all(np.isnan(eng.token_logprobs(8)[nb:]))
    finally:
        eng.set_token_logprobs(False)
    with pytest.raises(Exception):
        eng.token_logprobs(nb)                          # off: refused, not stale


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

        def run(temp):
            if temp > 0:
                eng.set_sampling(temp, 3, [stream_id(b, 0, 2) for b in range(nb)])
            try:
                seqs, lens, _ = eng.decode(_prompt(v, nb), max_length=3 + 20)
            finally:
                eng.set_sampling(0.0)
            return (seqs.copy(), lens.copy(), eng.avg_logprobs(nb).copy(),
                    eng.token_timestamps(nb, int(lens.max()) - 1, 3, nf).copy())

        for temp in (0.0, 0.6):
            off = run(temp)
            eng.set_token_logprobs(True)
            on = run(temp)
            assert not np.all(np.isnan(eng.token_logprobs(nb)))
            eng.set_token_logprobs(False)
            off2 = run(temp)
            for a, b, c in zip(off, on, off2):
                assert a.tobytes() == b.tobytes() == c.tobytes()
    finally:
        eng.close()


def test_native_seek_loop_equals_host_loop(tiny, engines):
    g, v, W, spec = tiny
    eng = engines["f32"]
    clips = [syn.synth_audio(60 + i, n, kind) for i, (n, kind) in
             enumerate([(480000, "mixed"), (130000, "noise"), (300001, "chirp"), (1600, "noise")])]
    _, nf = eng.mel(clips)
    sa, sb = {}, {}
    kw = dict(language="<|en|>", task="transcribe", max_new_tokens=40, return_token_logprobs=True)
    a = generation.generate(eng, len(clips), nf, stats=sa, native=True, **kw)
    b = generation.generate(eng, len(clips), nf, stats=sb, native=False, **kw)
    plain = generation.generate(eng, len(clips), nf, native=True, language="<|en|>", task="transcribe", max_new_tokens=40)
    assert sa == sb and sa["generate_calls"] > 1                      # a multi-pass clip
    assert "token_logprobs" not in plain and np.array_equal(plain["sequences"], a["sequences"])
    assert np.array_equal(a["sequences"], b["sequences"])
    for x, y, tx, ty, tp in zip(a["token_logprobs"], b["token_logprobs"], a["token_timestamps"], b["token_timestamps"],
                                plain["token_timestamps"]):
        assert x.dtype == np.float32 and y.dtype == np.float32
        assert len(x) == len(tx) == len(y) and np.array_equal(tx, ty) and np.array_equal(tx, tp)
        assert x.tobytes() == y.tobytes()
        assert not np.any(np.isnan(x)) and np.all(x <= 0)
    for segs, lp in zip(b["segments"], b["token_logprobs"]):
        assert sum(len(s.token_logprobs) for s in segs) == len(lp)


def _gold_clip(c):
    return syn.synth_audio(c["clip"]["seed"], int(round(c["clip"]["secs"] * 16000)), c["clip"]["kind"])


@pytest.mark.parametrize("dt", DTYPES)
def test_against_transformers(tiny, engines, dt):
    """transformers' greedy and 5-beam sequences, scored by one teacher-forced forward of transformers itself
    (tests/golden/gen_golden_token_logprobs.py).  f32: the free-running greedy / beam decode produces those tokens word for word
    and its values lie within the f32 bound of tests/test_gpu_score_vs_transformers.py; 16-bit engines: teacher-forced through
    cw_decode(forced=...), within that file's f16 / bf16 bounds -- the same quantity on the same model."""
    g, v, W, spec = tiny
    eng = engines[dt]
    assert GOLD["init"] == [v.sot, v.lang_id("en"), v.transcribe] and GOLD["eos"] == v.eos
    assert {c["search"] for c in GOLD["cases"]} == {"greedy", "beam5"}
    bound = BOUND[LONG[dt]]
    worst = 0.0
    for c in GOLD["cases"]:
        ids, ref = np.asarray(c["ids"], np.int64), np.asarray(c["logprob"], np.float64)
        _, nf = eng.mel([_gold_clip(c)])
        if dt == "f32":
            out = generation.generate(eng, 1, nf, language="<|en|>", task="transcribe", max_new_tokens=c["max_new_tokens"],
                                      num_beams=c["num_beams"], return_token_logprobs=True)
            assert out["sequences"][0].tolist() == ids.tolist(), (c["clip"], c["search"])
            got = out["token_logprobs"][0]
        else:
            eng.encode([0], [0], [3000])
            forced = np.full((1, 3 + len(ids)), -1, np.int32)
            forced[0, 3:] = ids
            eng.set_token_logprobs(True)
            try:
                seqs, lens, _ = eng.decode(_prompt(v, 1), max_length=3 + len(ids), forced=forced)
                got = eng.token_logprobs(1)[0, 3:3 + len(ids)]
            finally:
                eng.set_token_logprobs(False)
            assert seqs[0, 3:3 + len(ids)].tolist() == ids.tolist()
        d = np.abs(np.asarray(got, np.float64) - ref)
        print(dt, c["clip"]["seed"], c["search"], "max |logprob - ref| =", float(d.max()))
        worst = max(worst, float(d.max()))
        assert len(got) == len(ref) and np.all(d <= bound), (dt, c["clip"], c["search"], float(d.max()))
    print(dt, "worst", worst, "bound", bound)


@pytest.mark.parametrize("call", ["greedy", "beams", "prompt", "fallback"])
def test_pipeline_word_logprobs(tiny, call, monkeypatch):
    """A 70 s clip with strides at batch 2: every word carries a finite logprob <= 0, equal to the sum of generate's token values
    over the collator's groups; text and timestamps are those of the call without return_scores."""
    g, v, W, spec = tiny
    x = syn.synth_audio(0, 70 * 16000, "mixed")
    gk = {"language": "<|en|>", "task": "transcribe", "max_new_tokens": 16, "num_beams": 1}
    if call == "beams":
        gk["num_beams"] = 5
    elif call == "prompt":
        gk["prompt_ids"] = np.array([v.startofprev, ord("h"), ord("i")], np.int64)
    elif call == "fallback":
        gk.update(temperature=(0.0, 0.6), compression_ratio_threshold=1.2, logprob_threshold=-1.0)
    pipe = cw.pipeline("automatic-speech-recognition", model=cw.ModelBundle(spec, W), tokenizer=collate.Vocabulary.from_synthetic(v),
                       chunk_length_s=30, batch_size=2, return_timestamps="word", torch_dtype="float32", device="cuda:0",
                       sampling_seed=11)
    try:
        plain = pipe(x, generate_kwargs=dict(gk))
        assert all("logprob" not in w for w in plain["chunks"])
        recorded = []
        orig = generation.generate

        def spy(*a, **k):
            out = orig(*a, **k)
            recorded.append((list(k["item_ids"]), out))
            return out

        monkeypatch.setattr(generation, "generate", spy)
        scored = pipe(x, generate_kwargs=dict(gk), return_scores=True)
        monkeypatch.undo()
        assert scored["text"] == plain["text"]
        assert [(w["text"], w["timestamp"]) for w in scored["chunks"]] == [(w["text"], w["timestamp"]) for w in plain["chunks"]]
        assert len(scored["chunks"]) > 3
        windows = audio.chunk_windows(len(x), 480000, 80000, 80000)
        assert len(windows) == 3 and len(recorded) == 2
        outputs, lps = {}, {}
        for idxs, out in recorded:
            for k, i in enumerate(idxs):
                n = len(out["token_timestamps"][k])
                assert len(out["token_logprobs"][k]) == n and out["token_logprobs"][k].dtype == np.float32
                outputs[i] = {"tokens": out["sequences"][k][:n], "token_timestamps": out["token_timestamps"][k],
                              "stride": tuple(t / 16000 for t in windows[i][2])}
                lps[i] = out["token_logprobs"][k]
        order = sorted(outputs)
        text, words, groups = collate.decode_asr(pipe.vocab, [dict(outputs[i]) for i in order], return_timestamps="word",
                                                 return_token_groups=True)
        flat = np.concatenate([lps[i] for i in order]).astype(np.float64)
        assert text == scored["text"] and len(words) == len(scored["chunks"])
        used = set()
        for w, grp in zip(scored["chunks"], groups):
            assert np.isfinite(w["logprob"]) and w["logprob"] <= 0
            assert w["logprob"] == float(np.sum(flat[grp]))
            used |= set(grp)
        toks = np.concatenate([outputs[i]["tokens"] for i in order])
        assert used and all(toks[i] < spec.eos_token_id for i in used)         # text tokens only; what a seam drops is in no group
        if call == "fallback":
            assert any(r["temperature_index"] > 0 for r in pipe.stats["fallback"])
        with pytest.raises(ValueError, match="word"):
            pipe(x, generate_kwargs=dict(gk), return_timestamps=True, return_scores=True)
    finally:
        pipe.engine.close()
