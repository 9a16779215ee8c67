"""Scoring of known transcripts on the device (score.hip, cw_score_tokens, cw_align_score_tokens, Engine.score_tokens,
CrisperWhisperPipeline.score / align(return_scores=True)).

* The scoring head (cw_test_score_head: LayerNorm with affine, vocabulary projection, log-softmax, target gather, arg-max)
  against float64.
* The scoring forward against the per-position loop on the same 16-bit engine, at 1, 8, 9, 33 and 64 ragged rows.
* rows_per_item 1, 2, 5: a candidate's scores do not depend on what shares the call.
* align(return_scores=True): timestamps bit-identical to align(), scores bit-identical to score().
* The f32 engine's running avg_logprob of a greedy decode (cw_get_avg_logprobs) against scoring the generated tokens.
* Refusals before a launch.

Error bound of the kernel test.  u = 2^-24.  The reference takes the f32 inputs, computes the LayerNorm in float64, rounds it
to the 16-bit type (a16) and multiplies by the embedding (already rounded on upload) in float64.
  (1) logit: an f32 MFMA accumulation of D products of 16-bit values (exact in f32): |l - l64| <= D u A, A = sum_k |a_k w_k|
      (n-term recursive summation, n u A).
  (2) the kernel's LayerNorm runs in f32: its value differs from the float64 one by at most 64 u relative (two D-term sums for
      mean and variance in 64 lanes of D / 64 terms plus 6 shuffle steps, rsqrt, three multiplies and an add: well under
      64 roundings).  An element that lies within that distance of a 16-bit rounding boundary may round the other way, one
      16-bit ulp off.  The test finds those elements from the float64 values and adds F = sum over them of ulp16(a_k) max_n |w_nk|.
  So E = D u A + F per logit.  logsumexp: moves by at most E_row = the largest E of the row, plus the f32 sum's own error:
  each lane adds at most V / 16 + 1 terms, then 4 + 4 shuffle merges and n_split <= 256 partials, every term one expf (<= 2 ulp)
  of an argument rounded once, |arg| u: relative (V / 16 + 270 + 3) u + 100 u for |arg| <= 100, and logf's own 2 ulp on the
  result.  logprob = l[target] - lse:  |err| <= E_target + E_row + (V / 16 + 400) u + 4 u (1 + |lse| + |l[target]|).
  top_id: the kernel may return any id whose float64 logit lies within 2 E_row of the float64 maximum, and exactly the lowest
  id of an exact tie (identical embedding rows give bit-identical logits: same operands, same MFMA sequence).
"""
import numpy as np
import pytest

import crisperwhisper_amd as cw
from crisperwhisper_amd import collate, generation, synthetic as syn
from crisperwhisper_amd.engine import Engine, EngineError
from tests import helpers as Hh

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TOKEN_BOUND = {"f16": 0.08, "bf16": 0.5}          # twice the teacher-forced logit bounds of test_teacher_forced_decoder


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
def _ln16(x, g, b, dtype):
    """float64 LayerNorm rounded to the 16-bit type, and per element whether the f32 kernel may round the other way."""
    x = x.astype(np.float64)
    mean = x.mean(axis=1, keepdims=True)
    var = ((x - mean) ** 2).mean(axis=1, keepdims=True)
    a = (x - mean) / np.sqrt(var + 1e-5) * g.astype(np.float64) + b.astype(np.float64)
    a16 = _round16(a.astype(np.float32), dtype).astype(np.float64)
    mant = 7 if dtype == "bf16" else 10
    ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(a16), 2.0 ** -14))) - mant)
    to_boundary = np.abs(np.abs(a - a16) - ulp / 2)
    risky = to_boundary <= 64 * U * np.abs(a) + 2.0 ** -40
    return a16, ulp * risky


def _check_head(eng, dtype, x, g, b, emb, targets, ties=()):
    M, D = x.shape
    V = emb.shape[0]
    lp, ti, tl = eng.test_score_head(x, g, b, emb, targets)
    a16, flip = _ln16(x, g, b, dtype)
    w = emb.astype(np.float64)
    l64 = np.empty((M, V)); E = np.empty((M, V))
    wmax = np.abs(w).max(axis=0)
    F = (flip * wmax[None, :]).sum(axis=1)
    for n0 in range(0, V, 8192):
        ws = w[n0:n0 + 8192]
        l64[:, n0:n0 + 8192] = a16 @ ws.T
        E[:, n0:n0 + 8192] = D * U * (np.abs(a16) @ np.abs(ws).T) + F[:, None]
    mx = l64.max(axis=1)
    lse = mx + np.log(np.exp(l64 - mx[:, None]).sum(axis=1))
    rows = np.arange(M)
    lt = l64[rows, targets]
    Erow = E.max(axis=1)
    bound = E[rows, targets] + Erow + (V / 16 + 400) * U + 4 * U * (1 + np.abs(lse) + np.abs(lt))
    err = np.abs(lp.astype(np.float64) - (lt - lse))
    assert np.all(err <= bound), (dtype, M, V, int(np.argmax(err - bound)), float(err.max()), float(bound.min()))
    assert np.all((ti >= 0) & (ti < V))
    assert np.all(l64[rows, ti] >= mx - 2 * Erow), "top_id is not a maximum within the bound"
    err_t = np.abs(tl.astype(np.float64) - (l64[rows, ti] - lse))
    assert np.all(err_t <= 2 * Erow + (V / 16 + 400) * U + 4 * U * (1 + np.abs(lse) + np.abs(mx)))
    for m, lo in ties:
        assert ti[m] == lo, (m, int(ti[m]), lo)
    return lp, ti, tl, l64


def _head_case(dtype, M, D, V, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((M, D)) * 1.5 + 0.3).astype(np.float32)
    g = (1.0 + 0.1 * rng.standard_normal(D)).astype(np.float32)
    b = (0.05 * rng.standard_normal(D)).astype(np.float32)
    emb = (rng.standard_normal((V, D)) * 0.02).astype(np.float32)
    a16, _ = _ln16(x, g, b, dtype)
    targets = rng.integers(0, V, M).astype(np.int32)
    ties = []
    unit = lambda m: a16[m] / np.dot(a16[m], a16[m])
    targets[0] = min(3, V - 1)                                   # first tile
    # row 0 of x: the last id (the source row of the packed image's padding columns when V % 16 != 0) dominates, logit ~ 30:
    # padding columns that took part would add log(1 + their count) to the row's logsumexp
    emb[V - 1] = (unit(0) * 30.0).astype(np.float32)
    if M > 1:
        targets[1] = V - 1                                       # last valid column
        m = M - 1                                                # logits near +-60 in one row; its target is also the arg-max
        hi, lo = (V // 2, V // 2 + 1) if V > 4 else (0, 1)
        emb[hi] = (unit(m) * 60.0).astype(np.float32); emb[lo] = (-unit(m) * 60.0).astype(np.float32)
        targets[m] = hi
    if M > 2:
        targets[2] = max(0, ((V - 1) // 16) * 16)                # first column of the last tile
    if M > 4 and V > 40:                                         # exact two-way tie for the maximum of row 3: lowest id wins
        emb[7] = (unit(3) * 40.0).astype(np.float32)
        emb[V - 9] = emb[7]
        ties.append((3, 7))
    emb = _round16(emb, dtype)
    if ties:
        assert np.array_equal(emb[7], emb[V - 9])
    return x, g, b, emb, targets, ties


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("V", [48, 250])
@pytest.mark.parametrize("M", [1, 37, 130])
def test_score_head_vs_float64(tiny, dtype, M, V):
    g_, v_, W, spec = tiny
    eng = _engine(spec, W, dtype, rows=2)
    try:
        x, g, b, emb, targets, ties = _head_case(dtype, M, 128, V, 7000 + M + V)
        lp, ti, tl, l64 = _check_head(eng, dtype, x, g, b, emb, targets, ties)
        assert ti[0] == V - 1                                    # the planted row wins row 0 ...
        assert tl[0] > -1e-3                                     # ... and nearly all of its mass: no padding column shared it
        if M > 1:
            assert ti[M - 1] == targets[M - 1] and lp[M - 1] == tl[M - 1]
            assert np.isfinite(lp).all() and l64[M - 1].max() > 55 and l64[M - 1].min() < -55
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_score_head_full_vocabulary(tiny, dtype):
    g_, v_, W, spec = tiny
    eng = _engine(spec, W, dtype, rows=2)
    try:
        x, g, b, emb, targets, ties = _head_case(dtype, 64, 1280, 51866, 99)
        _check_head(eng, dtype, x, g, b, emb, targets, ties)
    finally:
        eng.close()


def test_score_head_refuses_bad_sizes(tiny):
    g_, v_, W, spec = tiny
    eng = _engine(spec, W, "bf16", rows=2)
    try:
        x = np.zeros((2, 64), np.float32); emb = np.zeros((20, 64), np.float32); one = np.ones(64, np.float32)
        with pytest.raises(EngineError):
            eng.test_score_head(x, one, one, emb, [0, 20])                         # target outside the vocabulary
        with pytest.raises(EngineError):
            eng.test_score_head(np.zeros((2, 48), np.float32), one[:48], one[:48], emb[:, :48], [0, 1])   # D % 32
    finally:
        eng.close()
    f32 = _engine(spec, W, "f32", rows=2)
    try:
        with pytest.raises(EngineError):
            f32.test_score_head(x, one, one, emb, [0, 1])
    finally:
        f32.close()


# ---------------------------------------------------------------------------------------------------------------- engine
def _ragged_rows(v, spec, n_rows, seed, longest=True):
    """n_rows decoder inputs: init + text + eos with 1 .. 444 text tokens (row 0 the shortest, row 1 the 448-position limit)."""
    rng = np.random.default_rng(seed)
    init = [v.sot, v.lang_id("en"), v.transcribe]
    lens = rng.integers(2, 40, n_rows)
    lens[0] = 1
    if n_rows > 1 and longest:
        lens[1] = spec.max_target_positions - len(init) - 1
    return [np.asarray(init + rng.integers(0, 256, n).tolist() + [v.eos], np.int64) for n in lens]


def _clips(n, seed=50):
    return [syn.synth_audio(seed + k, 16000 * (3 + k % 5), ("mixed", "noise", "chirp")[k % 3]) for k in range(n)]


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_score_prefill_vs_loop_ragged(tiny, dtype):
    g, v, W, spec = tiny
    eng = _engine(spec, W, dtype, rows=64)
    try:
        runs = 0
        for n_rows in (1, 8, 9, 33, 64):
            eng.mel(_clips(n_rows))
            rows = _ragged_rows(v, spec, n_rows, 300 + n_rows, longest=n_rows in (8, 33))
            eng.set_score_prefill(True)
            lp, ti, tl = eng.score_tokens(rows, 3)
            runs += 1
            assert eng.score_prefill_runs() == runs
            eng.set_score_prefill(False)
            lp2, ti2, tl2 = eng.score_tokens(rows, 3)
            assert eng.score_prefill_runs() == runs
            worst = 0.0
            agree = n = 0
            for r in range(n_rows):
                assert len(lp[r]) == len(rows[r]) - 3 == len(lp2[r])
                assert np.isfinite(lp[r]).all() and np.all(lp[r] <= 0) and np.all(tl[r] >= lp[r])
                worst = max(worst, float(np.abs(lp[r] - lp2[r]).max()), float(np.abs(tl[r] - tl2[r]).max()))
                agree += int((ti[r] == ti2[r]).sum()); n += len(ti[r])
            print(dtype, n_rows, "rows: worst |prefill - loop| =", worst, " top_id agreement", agree / n)
            assert worst <= TOKEN_BOUND[dtype], (n_rows, worst)
            assert agree >= 0.9 * n
    finally:
        eng.close()


def test_f32_engine_scores_through_the_loop(tiny):
    g, v, W, spec = tiny
    eng = _engine(spec, W, "f32", rows=4)
    try:
        eng.mel(_clips(3))
        rows = _ragged_rows(v, spec, 3, 11, longest=False)
        lp, ti, tl = eng.score_tokens(rows, 3)
        assert eng.score_prefill_runs() == 0
        lp1, ti1, tl1 = eng.score_tokens(rows[:1], 3)
        assert np.allclose(lp[0], lp1[0], atol=4e-3) and np.all(tl[0] >= lp[0])
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
def test_rows_per_item_independence(tiny, dtype):
    g, v, W, spec = tiny
    eng = _engine(spec, W, dtype, rows=16)
    try:
        clips = _clips(3, seed=70)
        cands = _ragged_rows(v, spec, 15, 5, longest=False)                   # 3 items x 5 candidates
        eng.mel(clips)
        lp5, ti5, tl5 = eng.score_tokens(cands, 3, rows_per_item=5)
        lp2, ti2, tl2 = eng.score_tokens([cands[0], cands[3], cands[5], cands[6], cands[10], cands[14]], 3, rows_per_item=2)
        for a, b in zip((0, 3, 5, 6, 10, 14), range(6)):
            _same(dtype, (lp5[a], ti5[a], tl5[a]), (lp2[b], ti2[b], tl2[b]))
        for item in range(3):                                                  # the same text sent alone
            eng.mel([clips[item]])
            k = item * 5 + 2
            lp1, ti1, tl1 = eng.score_tokens([cands[k]], 3, rows_per_item=1)
            _same(dtype, (lp5[k], ti5[k], tl5[k]), (lp1[0], ti1[0], tl1[0]))
        if dtype != "f32":
            assert eng.score_prefill_runs() == 5
    finally:
        eng.close()


def _same(dtype, a, b):
    if dtype == "f32":          # the loop's decode step picks kernels by batch size: equal within the f32 bound, not bit for bit
        assert np.allclose(a[0], b[0], atol=4e-3) and np.allclose(a[2], b[2], atol=4e-3)
    else:                       # the prefill: every row's arithmetic is its own
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])
        assert np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))


@pytest.mark.parametrize("dtype", ["bfloat16", "float16", "float32"])
def test_align_return_scores_matches_align_and_score(tiny, dtype):
    g, v, W, spec = tiny
    pipe = cw.pipeline("automatic-speech-recognition", model=cw.ModelBundle(spec, W), tokenizer=collate.Vocabulary.from_synthetic(v),
                       batch_size=4, return_timestamps="word", torch_dtype=dtype, device="cuda:0")
    try:
        clips = _clips(3, seed=90)
        texts = [[ord(c) for c in t] for t in (" abc def ghi", " hello, world", " a")]
        kw = dict(language="<|en|>", task="transcribe")
        plain = pipe.align(clips, texts, **kw)
        scored = pipe.align(clips, texts, return_scores=True, **kw)
        only = pipe.score(clips, texts, **kw)
        for p, s, o in zip(plain, scored, only):
            assert p["text"] == s["text"] == o["text"]
            assert [(c["text"], c["timestamp"]) for c in p["chunks"]] == [(c["text"], c["timestamp"]) for c in s["chunks"]]
            assert [c["logprob"] for c in s["chunks"]] == [c["logprob"] for c in o["chunks"]]
            assert s["logprob"] == o["logprob"] and s["avg_logprob"] == o["avg_logprob"]
            assert o["logprob"] == pytest.approx(sum(t["logprob"] for t in o["tokens"]))
        eng = pipe.engine
        _, nf = eng.mel(clips)
        rows = [np.asarray([v.sot, v.lang_id("en"), v.transcribe] + t + [v.eos], np.int64) for t in texts]
        ts = eng.align_tokens(nf, rows, 3)
        ts2, lp, ti, tl = eng.align_score_tokens(nf, rows, 3)
        lp3, ti3, tl3 = eng.score_tokens(rows, 3)
        for r in range(3):
            assert np.array_equal(ts[r].view(np.uint32), ts2[r].view(np.uint32))
            assert np.array_equal(lp[r].view(np.uint32), lp3[r].view(np.uint32)) and np.array_equal(ti[r], ti3[r])
    finally:
        pipe.engine.close()


def test_avg_logprob_of_greedy_decode_matches_scoring(tiny):
    """cw_get_avg_logprobs (the mean over the generated tokens of log_softmax of the PROCESSED scores at the token) against the
    scores of the generated tokens on the f32 engine.

    The exact relation.  Processing masks a set S of ids (suppress lists, timestamp rules) to -inf and changes nothing else, so
    at every position  processed = raw - log(1 - p_S)  with p_S the raw probability mass of S.  The two are therefore NOT equal
    merely because no masked id is the arg-max (the premise the issue states); they are equal within a bound only where p_S is
    below it.  The generated token t is unmasked, so p_S <= 1 - p_t... and with t the raw arg-max (checked from top_id),
    0 <= processed - raw <= -log(p_top) = -top_logprob.  A case therefore counts when every generated token is the raw arg-max
    AND the mean of -top_logprob over its tokens is <= 4e-3: then |avg - scored| <= 4e-3 (mass) + 4e-3 (the f32 per-token
    bound, twice the logit bound 2e-3) is asserted, two-sided.

    The first generated token is a special case with an exact value: the timestamp rules mask every text id there, so it is never
    the raw arg-max of a text model; here all timestamp logits are equal (zero rows), the rules leave the
    max_initial_timestamp_index + 1 first timestamps, and the processed log-probability of the chosen one is exactly
    -log(max_initial_timestamp_index + 1).  The expected average is therefore (-log(51) + the scored sum of tokens 2 .. n) / n,
    and the arg-max and mass conditions apply to tokens 2 .. n.

    The random tiny model is far too flat for that (its arg-max carries e^-2 .. e^-3 of the mass), so the cases use a peaked
    variant of it: the embedding rows of the non-text ids (eos, tags, timestamps:
    the only ids the timestamp rules and this spec's empty suppress lists can mask) are zero, pinning their logits to 0, and
    the text rows are scaled up until the best text logit leaves the 1513 zero logits no mass.  Generations run into max_length
    (the zero eos row never wins), so the decode counts its n generated tokens and sum / n is compared with the scored
    sum over the same n tokens / n: Whisper's sum / (length + 1) with the eos counted where it is generated, which is how
    cw_get_avg_logprobs counts."""
    import dataclasses
    g, v, W0, spec = tiny
    init = [v.sot, v.lang_id("en"), v.transcribe, v.notimestamps]
    kept = 0
    for scale in (8.0, 24.0):
        W = dict(W0)
        emb = np.array(W["model.decoder.embed_tokens.weight"], np.float32, copy=True)
        emb[:v.eos] *= scale
        emb[v.eos:] = 0.0
        W["model.decoder.embed_tokens.weight"] = emb
        eng = _engine(dataclasses.replace(spec, suppress_tokens=(), begin_suppress_tokens=()), W, "f32", rows=8)
        try:
            for max_length in (6, 12):
                eng.mel(_clips(8, seed=120))
                eng.encode(list(range(8)), [0] * 8, [3000] * 8)
                eng.set_thresholds(logprob_threshold=-1.0)
                seq, lens, _ = eng.decode(np.tile(np.asarray(init, np.int32), (8, 1)), max_length=max_length)
                avg = eng.avg_logprobs(8)
                eng.set_thresholds(None)
                rows, n_gen = [], []
                for r in range(8):
                    gen = seq[r, 4:lens[r]].astype(np.int64)
                    ended = len(gen) > 0 and gen[-1] == v.eos
                    rows.append(np.concatenate([init, gen if ended else np.concatenate([gen, [v.eos]])]))
                    n_gen.append(len(gen))
                lp, ti, tl = eng.score_tokens(rows, 4)
                for r in range(8):
                    n = n_gen[r]
                    first = int(rows[r][4])
                    if n < 2 or not (v.timestamp_begin <= first <= v.timestamp_begin + spec.max_initial_timestamp_index) or \
                            not np.array_equal(ti[r][1:n], rows[r][5:4 + n]):
                        print("scale", scale, "max_length", max_length, "row", r, "skipped: generated", rows[r][4:4 + n].tolist(),
                              "raw arg-max", ti[r][:n].tolist())
                        continue                  # a masked id was the raw arg-max somewhere
                    mass = float(-tl[r][1:n].astype(np.float64).mean())
                    raw = (-np.log(spec.max_initial_timestamp_index + 1.0) + float(lp[r][1:n].astype(np.float64).sum())) / n
                    print("scale", scale, "max_length", max_length, "row", r, n, "tokens: decode", float(avg[r]), "scored", raw,
                          "mean -top_logprob", mass)
                    if mass > 4e-3:
                        continue                  # the masked ids may carry more than the bound: the definitions differ
                    assert abs(float(avg[r]) - raw) <= 8e-3, (scale, max_length, r, float(avg[r]), raw)
                    kept += 1
        finally:
            eng.close()
    assert kept >= 1


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_refusals_before_a_launch(tiny, dtype):
    import ctypes as C
    g, v, W, spec = tiny
    eng = _engine(spec, W, dtype, rows=4)
    try:
        eng.mel(_clips(2))
        init = [v.sot, v.lang_id("en"), v.transcribe]
        good = np.asarray(init + [5, 6, v.eos], np.int64)
        runs = eng.score_prefill_runs()
        with pytest.raises(ValueError):
            eng.score_tokens([np.asarray(init + [g.vocab, v.eos])], 3)                       # id outside the vocabulary
        with pytest.raises(EngineError):
            eng.score_tokens([np.asarray(init + [5, v.eos, 6, v.eos])], 3)                   # eos inside
        with pytest.raises(EngineError):
            eng.score_tokens([good], 3, rows_per_item=0)
        with pytest.raises(EngineError):
            eng.score_tokens([good] * 6, 3, rows_per_item=3)                                 # 6 rows, max_batch 4
        with pytest.raises(EngineError):
            eng.score_tokens([np.asarray(init)], 3)                                          # no eos: fewer than n_init + 1 ids
        tab = np.ascontiguousarray(good[None].astype(np.int32)); n = np.asarray([len(good)], np.int32)
        P = lambda a: a.ctypes.data_as(C.c_void_p)
        out = np.zeros(8, np.float32)
        for bad_id in (g.vocab, -1):                                                         # past Python's own check, in the C ABI
            bad = tab.copy(); bad[0, 4] = bad_id
            assert eng.lib.cw_score_tokens(eng.ctx, 1, 1, P(bad), len(good), P(n), 3, P(out), None, None) != 0
            assert "outside the vocabulary" in eng.lib.cw_last_error(eng.ctx).decode()
        assert eng.lib.cw_score_tokens(eng.ctx, 1, 1, P(tab), len(good), P(n), 3, None, None, None) != 0     # null output
        assert eng.lib.cw_score_tokens(eng.ctx, 1, 1, None, len(good), P(n), 3, P(np.zeros(8, np.float32)), None, None) != 0
        assert eng.score_prefill_runs() == runs
        lp, ti, tl = eng.score_tokens([good], 3)                                             # and the context still works
        assert np.isfinite(lp[0]).all()
    finally:
        eng.close()
