"""Alignment scores on the device (cw_set_alignment_scores; align_path_score_kernel in csrc/align.hip): the kernel against the
float64 definition of tests/alignment_score_refs.py through cw_test_align_path_scores, bit-identity of a row across batches and
runs, the engine's timestamp stage after greedy, beam, forced and native seek-loop decoding recomputed in float64 from the rows
and timestamps the engine itself returns, the switch leaving every existing output alone, and the pipeline's word values."""
import numpy as np
import pytest

import crisperwhisper_amd as cw
from crisperwhisper_amd import collate, generation, synthetic as syn
from crisperwhisper_amd.engine import Engine, EngineError
from tests import alignment_score_refs as R
from tests import helpers as Hh

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tiny():
    return Hh.tiny_setup()


@pytest.fixture(scope="module")
def engines(tiny):
    g, v, W, spec = tiny
    out = {}
    for dt in ("f32", "bf16"):
        e = Engine(spec, dtype=dt, max_batch=8)
        e.load_state_dict(W)
        out[dt] = e
    yield out
    for e in out.values():
        e.close()


# ------------------------------------------------------------------------------------------------------------------ kernel
def _rows(rng, B, Ha, N, S, n_cols, kind):
    """attn [B][Ha][N][S] and first_col [B][N] for one of the input families; frames at or beyond n_cols[b] hold 7.0 (stale
    data that must not count)."""
    attn = np.full((B, Ha, N, S), 7.0, np.float32)
    fc = np.zeros((B, N), np.int32)
    for b in range(B):
        n = n_cols[b]
        if n > 0:
            cuts = np.sort(rng.integers(0, n, N)).astype(np.int32)          # a monotone path; equal neighbours happen
            fc[b] = cuts
        if kind == "random":
            attn[b, :, :, :n] = np.exp(rng.uniform(0.0, np.log(1e4), (Ha, N, n))).astype(np.float32)     # 1e4 dynamic range
        elif kind == "onehot":
            attn[b, :, :, :n] = 0.0
            if n > 0:
                for i in range(N):
                    attn[b, :, i, 0 if i % 2 == 0 else n - 1] = 0.5 + i
        elif kind == "zero_row":
            attn[b, :, :, :n] = rng.uniform(0.5, 1.5, (Ha, N, n)).astype(np.float32)
            attn[b, Ha - 1, N // 2, :n] = 0.0                                # one head saw nothing for one token
        elif kind == "equal_fc":
            attn[b, :, :, :n] = rng.uniform(0.0, 1.0, (Ha, N, n)).astype(np.float32)
            fc[b] = fc[b, 0]                                                 # every token starts on one frame
    return attn, fc


# Tolerances (tests/alignment_score_refs.py: mass_tolerance, spread_interval), u = 2^-24, n = n_cols:
#   mass    W / T is a ratio of two sums of n non-negative float32 terms.  Summed in float32 in any order, each sum carries a
#           relative error below n u, so the ratio is off by at most 2 n u relatively, and it is at most 1: |error| <= 2 n u.
#   spread  var = V / T with V = sum_j w[j] (j - mu)^2, again sums of non-negative terms: the same bound applied to the variance,
#           var (1 - 2 n u) <= var' <= var (1 + 2 n u).  The square root is monotone, so
#               0.02 sqrt(var (1 - 2 n u)) <= spread' <= 0.02 sqrt(var (1 + 2 n u)),
#           i.e. a relative error of about n u in the spread; the result is rounded to float32 once more (the factors 1 -+ 2 u).
#           A variance of 0 (a one-hot row) leaves no room: the spread is 0.  The only other slack is the float64 reference's own
#           error in its centre (n^2 2^-53 frames, squared), 1e-21 frames^2 at n = 1500.
#   NaN positions match exactly.
def _check(eng, attn, fc, n_cols, collar, where, onehot=False):
    mass, spread = eng.test_align_path_scores(attn, n_cols, fc, collar)
    assert mass.shape == spread.shape == fc.shape and mass.dtype == np.float32
    if onehot:                                               # every row has all its weight on one frame: no spread, exactly
        for b in range(attn.shape[0]):
            assert np.all(spread[b] == 0.0) if n_cols[b] > 0 else np.all(np.isnan(spread[b])), (where, b, spread[b])
            assert np.all((mass[b] == 0.0) | (mass[b] == 1.0)) if n_cols[b] > 0 else np.all(np.isnan(mass[b])), (where, b, mass[b])
    worst = 0.0
    for b in range(attn.shape[0]):
        worst = max(worst, R.check_against(mass[b], spread[b], attn[b], n_cols[b], fc[b], collar, where=f"{where} b={b}"))
    return mass, spread, worst


N_COLS = [0, 1, 3, 63, 65, 257, 749]


@pytest.mark.parametrize("kind", ["random", "onehot", "zero_row", "equal_fc"])
@pytest.mark.parametrize("S", [8, 260, 1500])
def test_kernel_against_float64(engines, S, kind):
    """Every n_cols of the list that fits S, and n_cols == S; N in {1, 2, 5}; Ha in {1, 3}; B in {1, 3} with a different n_cols
    per item; collar in {0, 2, n_cols}.  NaN positions exactly, values within the bounds of alignment_score_refs."""
    eng = engines["f32"]
    rng = np.random.default_rng(S * 10 + len(kind))
    ns = [n for n in N_COLS if n <= S] + [S]
    worst, cases = 0.0, 0
    for k, n in enumerate(ns):
        N, Ha = (1, 2, 5)[k % 3], (1, 3)[k % 2]
        for B in (1, 3):
            n_cols = [n] if B == 1 else [n, ns[(k + 1) % len(ns)], ns[(k + 3) % len(ns)]]
            attn, fc = _rows(rng, B, Ha, N, S, n_cols, kind)
            for collar in (0, 2, n):
                _, _, w = _check(eng, attn, fc, n_cols, collar, f"{kind} S={S} n={n_cols} N={N} Ha={Ha} collar={collar}",
                                 onehot=kind == "onehot")
                worst = max(worst, w)
                cases += 1
    # every combination of N and Ha at one odd size, more than one block (B * N = 15 rows over blocks of 4 waves)
    n = min(S, 65)
    for N in (1, 2, 5):
        for Ha in (1, 3):
            attn, fc = _rows(rng, 3, Ha, N, S, [n, max(n - 2, 0), min(S, 3)], kind)
            _, _, w = _check(eng, attn, fc, [n, max(n - 2, 0), min(S, 3)], 2, f"{kind} S={S} N={N} Ha={Ha}", onehot=kind == "onehot")
            worst = max(worst, w)
    print(f"{kind} S={S}: {cases} cases, worst |mass - float64| = {worst:.3e}")


def test_kernel_edge_values(engines):
    eng = engines["f32"]
    S, n = 260, 65
    attn = np.zeros((1, 3, 3, S), np.float32)
    attn[0, :, 0, 0] = 2.0                                   # one-hot at frame 0
    attn[0, :, 1, n - 1] = 3.0                               # one-hot at frame n - 1
    attn[0, :, 2, :n] = 0.25                                 # uniform
    fc = np.array([[0, 40, 50]], np.int32)
    mass, spread = eng.test_align_path_scores(attn, [n], fc, 0)
    assert mass[0, 0] == 1.0 and spread[0, 0] == 0.0
    assert mass[0, 1] == 0.0 and spread[0, 1] == 0.0         # all of it on frame 64, the path says 40 .. 49
    assert abs(float(mass[0, 2]) - 15 / 65) <= R.mass_tolerance(n)
    assert abs(float(spread[0, 2]) - 0.02 * np.sqrt((n * n - 1) / 12.0)) <= 1e-6
    mass, _ = eng.test_align_path_scores(attn, [n], fc, n)
    assert mass[0].tolist() == [1.0, 1.0, 1.0]               # a collar of n_cols covers every frame
    fc[0, 1] = -1                                            # no first frame: NaN for that token alone
    mass, spread = eng.test_align_path_scores(attn, [n], fc, 0)
    assert np.isnan(mass[0]).tolist() == [False, True, False] and np.isnan(spread[0]).tolist() == [False, True, False]
    with pytest.raises(EngineError):
        eng.test_align_path_scores(attn, [n], fc, -1)
    with pytest.raises(EngineError):
        eng.test_align_path_scores(attn, [S + 1], fc, 0)
    with pytest.raises(EngineError):
        eng.test_align_path_scores(attn[..., :258], [n], fc, 0)             # S no multiple of 4


@pytest.mark.parametrize("fill", [np.nan, 1e30])
def test_frames_behind_n_cols_never_count(engines, fill):
    eng = engines["f32"]
    rng = np.random.default_rng(5)
    S, n_cols = 260, [63, 257, 1]
    attn, fc = _rows(rng, 3, 3, 5, S, n_cols, "random")
    want = eng.test_align_path_scores(attn, n_cols, fc, 2)
    for b, n in enumerate(n_cols):
        attn[b, :, :, n:] = fill
    got = eng.test_align_path_scores(attn, n_cols, fc, 2)
    assert not np.any(np.isnan(want[0])) and not np.any(np.isnan(want[1]))
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


def test_a_row_has_the_same_bits_alone_in_a_batch_and_run_to_run(engines):
    eng = engines["f32"]
    rng = np.random.default_rng(9)
    S, n_cols = 1500, [749, 1500, 65]
    attn, fc = _rows(rng, 3, 3, 5, S, n_cols, "random")
    m3, s3 = eng.test_align_path_scores(attn, n_cols, fc, 2)
    m3b, s3b = eng.test_align_path_scores(attn, n_cols, fc, 2)
    assert m3.tobytes() == m3b.tobytes() and s3.tobytes() == s3b.tobytes()
    for b in range(3):
        m1, s1 = eng.test_align_path_scores(attn[b:b + 1], n_cols[b:b + 1], fc[b:b + 1], 2)
        assert m1[0].tobytes() == m3[b].tobytes() and s1[0].tobytes() == s3[b].tobytes()


# ------------------------------------------------------------------------------------------------------------------ engine
COLLAR = 2
CLIPS = [(2.0, "noise"), (3.1, "mixed")]                     # two lengths: a different n_cols per row


def _clips():
    return [syn.synth_audio(700 + i, int(s * 16000), kind) for i, (s, kind) in enumerate(CLIPS)]


def _prompt(v, nb):
    return np.tile(np.array([[v.sot, v.lang_id("en"), v.transcribe]], np.int32), (nb, 1))


def _check_stage(eng, nb, L, n_prompt, nf, token_ts, lens=None, where=""):
    """The scores of the last timestamp stage against float64 on the rows and timestamps the engine returns: row b's token rows
    are positions n_prompt .. L_b - 1 (L_b = lens[b] - 1, default L), their first frames token_ts / 0.02."""
    mass, spread = eng.alignment_scores(nb, L)
    rows = eng.alignment(nb, L)
    n_cols = R.timestamp_ncols(nf)
    assert mass.shape == spread.shape == (nb, L + 1)
    n_vals = 0
    for b in range(nb):
        Lb = L if lens is None else int(lens[b]) - 1
        assert np.all(np.isnan(mass[b, :n_prompt])) and np.all(np.isnan(spread[b, :n_prompt]))       # prompt positions
        assert np.all(np.isnan(mass[b, Lb:])) and np.all(np.isnan(spread[b, Lb:]))                 # the eos slot and beyond
        if Lb <= n_prompt:
            continue
        fc = np.rint(np.asarray(token_ts[b][n_prompt:Lb], np.float64) / 0.02).astype(np.int64)
        R.check_against(mass[b, n_prompt:Lb], spread[b, n_prompt:Lb], rows[b][:, n_prompt:Lb], n_cols[b], fc, COLLAR,
                        where=f"{where} row {b}")
        ok = ~np.isnan(mass[b, n_prompt:Lb])
        assert np.all((mass[b, n_prompt:Lb][ok] >= 0) & (mass[b, n_prompt:Lb][ok] <= 1 + R.mass_tolerance(n_cols[b])))
        n_vals += int(ok.sum())
    return mass, spread, n_vals


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_engine_greedy_beam_and_forced(tiny, engines, dt):
    g, v, W, spec = tiny
    eng = engines[dt]
    nb, steps = 2, 9
    _, nf = eng.mel(_clips())
    assert nf[0] != nf[1]
    eng.set_alignment_scores(True, COLLAR)
    try:
        # greedy
        eng.encode(list(range(nb)), [0] * nb, [3000] * nb)
        seqs, lens, _ = eng.decode(_prompt(v, nb), max_length=3 + steps)
        L = int(lens.max()) - 1
        ts = eng.token_timestamps(nb, L, 3, nf)
        m, s, n_vals = _check_stage(eng, nb, L, 3, nf, ts, where=f"{dt} greedy")
        assert n_vals > 0
        m2, s2 = eng.alignment_scores(nb, L + 3)                            # a wider frame: NaN behind the rows
        assert m2[:, :L + 1].tobytes() == m.tobytes() and np.all(np.isnan(m2[:, L + 1:])) and np.all(np.isnan(s2[:, L + 1:]))
        with pytest.raises(EngineError):
            eng.alignment_scores(nb + 1, L)                                 # more rows than were scored
        with pytest.raises(EngineError):
            eng.alignment_scores(nb, L - 1)
        # beam search with 2 beams: the timestamp stage reads the beam-gathered copy of the rows
        eng.encode(list(range(nb)), [0] * nb, [3000] * nb)
        bs, _, Lb, _ = generation.beam_search(eng, _prompt(v, nb), 3 + steps, 0, 2)
        ts = eng.token_timestamps(nb, Lb, 3, nf)
        _, _, n_vals = _check_stage(eng, nb, Lb, 3, nf, ts, where=f"{dt} beam")
        assert n_vals > 0
        # forced alignment of rows of two lengths: each row over its own token count
        rng = np.random.default_rng(3)
        init = [v.sot, v.lang_id("en"), v.transcribe]
        ids = [np.concatenate([init, rng.integers(0, 256, n), [v.eos]]).astype(np.int64) for n in (8, 5)]
        ats = eng.align_tokens(nf, ids, 3)
        Lmax = max(len(r) for r in ids) - 1
        fm, fs, n_vals = _check_stage(eng, nb, Lmax, 3, nf, ats, lens=[len(r) for r in ids], where=f"{dt} align_tokens")
        assert n_vals == 8 + 5                                              # softmax rows are positive: every text token has a value
        # ... and together with the scoring forward: the same rows, the same values
        ats2 = eng.align_score_tokens(nf, ids, 3)[0]
        gm, gs = eng.alignment_scores(nb, Lmax)
        assert all(np.array_equal(a, b) for a, b in zip(ats, ats2))
        assert gm.tobytes() == fm.tobytes() and gs.tobytes() == fs.tobytes()
    finally:
        eng.set_alignment_scores(False)
    with pytest.raises(EngineError):
        eng.alignment_scores(nb, Lmax)                                      # off: refused, not stale
    with pytest.raises(EngineError):
        eng.set_alignment_scores(True, -1)
    # refused while a beam search is open
    eng.encode(list(range(nb)), [0] * nb, [3000] * nb)
    eng.beam_begin(_prompt(v, nb), 2, 3 + steps)
    try:
        with pytest.raises(EngineError, match="beam"):
            eng.set_alignment_scores(True, COLLAR)
        eng.set_alignment_scores(False)                                     # switching off changes nothing: never refused
    finally:
        eng.decode(_prompt(v, nb), max_length=4)                            # a plain decode closes the search


def test_a_search_left_open_does_not_block_later_calls(tiny, engines):
    """A beam search that was interrupted (an exception between beam_begin and beam_finish) leaves the engine as usable as it
    was before the switch existed: generate and align without the flag run, with and without the switch having been on, and
    once a decode has closed the search the flag is served again."""
    g, v, W, spec = tiny
    eng = engines["f32"]
    nb = 2
    _, nf = eng.mel(_clips())
    kw = dict(language="<|en|>", task="transcribe", max_new_tokens=9)
    want = generation.generate(eng, nb, nf, **kw)
    for was_on in (False, True):
        eng.set_alignment_scores(was_on, COLLAR)
        eng.encode(list(range(nb)), [0] * nb, [3000] * nb)
        eng.beam_begin(_prompt(v, nb), 2, 3 + 9)
        eng.beam_step(4)                                                    # ... and the caller never comes back
        got = generation.generate(eng, nb, nf, **kw)
        assert np.array_equal(got["sequences"], want["sequences"]) and "alignment_scores" not in got
        assert all(np.array_equal(a, b) for a, b in zip(got["token_timestamps"], want["token_timestamps"]))
        assert eng.alignment_scores_on is False
        eng.beam_begin(_prompt(v, nb), 2, 3 + 9)
        ids = [np.asarray(s[:4], np.int64) for s in want["sequences"]]
        ids = [t[t < spec.eos_token_id] for t in ids]
        al = generation.align(eng, nb, nf, ids, language="<|en|>", task="transcribe")
        assert len(al["token_timestamps"]) == nb and "alignment_scores" not in al
    scored = generation.generate(eng, nb, nf, return_alignment_scores=True, alignment_collar_frames=COLLAR, **kw)
    assert np.array_equal(scored["sequences"], want["sequences"]) and len(scored["alignment_scores"]) == nb
    eng.set_alignment_scores(False)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_native_seek_loop_equals_the_checked_host_loop(tiny, engines, dt, monkeypatch):
    """A clip that needs two seek passes: every pass of the host loop is checked against float64, and the native loop
    (cw_transcribe) returns the same bits, sliced and eos-stripped like its tokens."""
    g, v, W, spec = tiny
    eng = engines[dt]
    clips = [syn.synth_audio(60, 480000, "mixed"), syn.synth_audio(62, 300001, "chirp")]
    _, nf = eng.mel(clips)
    kw = dict(language="<|en|>", task="transcribe", max_new_tokens=12, return_alignment_scores=True, alignment_collar_frames=COLLAR)
    checked = []
    orig = eng.token_timestamps

    def spy(nb, L, n_prompt, num_frames):
        ts = orig(nb, L, n_prompt, num_frames)
        checked.append(_check_stage(eng, nb, L, n_prompt, num_frames, ts, where=f"{dt} pass {len(checked)}")[2])
        return ts

    monkeypatch.setattr(eng, "token_timestamps", spy)
    sb = {}
    b = generation.generate(eng, len(clips), nf, stats=sb, native=False, **kw)
    monkeypatch.undo()
    sa = {}
    a = generation.generate(eng, len(clips), nf, stats=sa, native=True, **kw)
    plain = generation.generate(eng, len(clips), nf, native=True, language="<|en|>", task="transcribe", max_new_tokens=12)
    assert sa == sb and sa["generate_calls"] >= 2 and len(checked) == sb["generate_calls"] and sum(checked) > 0
    assert "alignment_scores" not in plain and np.array_equal(plain["sequences"], a["sequences"])
    assert np.array_equal(a["sequences"], b["sequences"])
    for k in range(len(clips)):
        n = len(a["token_timestamps"][k])
        assert np.array_equal(a["token_timestamps"][k], b["token_timestamps"][k])
        assert np.array_equal(a["token_timestamps"][k], plain["token_timestamps"][k])
        for key in ("alignment_scores", "alignment_spreads"):
            assert a[key][k].dtype == np.float32 and len(a[key][k]) == len(b[key][k]) == n
            assert a[key][k].tobytes() == b[key][k].tobytes()
    for segs, m in zip(b["segments"], b["alignment_scores"]):
        assert sum(len(s.alignment_scores) for s in segs) == len(m)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_the_switch_changes_no_existing_output(tiny, dt):
    g, v, W, spec = tiny
    eng = Engine(spec, dtype=dt, max_batch=4)
    try:
        eng.load_state_dict(W)
        nb = 2
        _, nf = eng.mel(_clips())
        eng.encode(list(range(nb)), [0] * nb, [3000] * nb)
        eng.set_token_logprobs(True)

        def run():
            seqs, lens, _ = eng.decode(_prompt(v, nb), max_length=3 + 9)
            return (seqs.copy(), lens.copy(), eng.token_timestamps(nb, int(lens.max()) - 1, 3, nf).copy(),
                    eng.token_logprobs(nb).copy())

        off = run()
        eng.set_alignment_scores(True, COLLAR)
        on = run()
        assert not np.all(np.isnan(eng.alignment_scores(nb, int(on[1].max()) - 1)[0]))
        eng.set_alignment_scores(False)
        off2 = run()
        for a, b, c in zip(off, on, off2):
            assert a.tobytes() == b.tobytes() == c.tobytes()
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------- pipeline
def test_pipeline_words_carry_both_keys(tiny, monkeypatch):
    """A 70 s clip with strides at batch 2 (seam merges), greedy: every chunk gains both keys, each the float64 mean of
    generate's token values over the collator's groups; text and timestamps are those of the call without the flag.  Then a
    single window decoded in one pass: pipe.align of that call's own transcript returns the same values."""
    g, v, W, spec = tiny
    vocab = collate.Vocabulary.from_synthetic(v)
    gk = {"language": "<|en|>", "task": "transcribe", "max_new_tokens": 16, "num_beams": 1}
    pipe = cw.pipeline("automatic-speech-recognition", model=cw.ModelBundle(spec, W), tokenizer=vocab, chunk_length_s=30,
                       batch_size=2, return_timestamps="word", torch_dtype="float32", device="cuda:0")
    try:
        x = syn.synth_audio(0, 70 * 16000, "mixed")
        plain = pipe(x, generate_kwargs=dict(gk))
        assert all(set(w) == {"text", "timestamp"} for w in plain["chunks"])
        recorded = []
        orig = generation.generate

        def spy(*a, **k):
            out = orig(*a, **k)
            recorded.append((list(k["item_ids"]), out))
            return out

        monkeypatch.setattr(generation, "generate", spy)
        scored = pipe(x, generate_kwargs=dict(gk), return_alignment_scores=True)
        assert scored["text"] == plain["text"] and len(scored["chunks"]) > 3
        assert [(w["text"], w["timestamp"]) for w in scored["chunks"]] == [(w["text"], w["timestamp"]) for w in plain["chunks"]]
        for w in scored["chunks"]:
            assert set(w) == {"text", "timestamp", "alignment_score", "alignment_spread"}
            assert 0.0 <= w["alignment_score"] <= 1.0 and np.isfinite(w["alignment_spread"]) and w["alignment_spread"] >= 0
        from crisperwhisper_amd import audio
        windows = audio.chunk_windows(len(x), 480000, 80000, 80000)
        outputs, mass, spread = {}, {}, {}
        for idxs, out in recorded:
            for k, i in enumerate(idxs):
                n = len(out["token_timestamps"][k])
                assert len(out["alignment_scores"][k]) == len(out["alignment_spreads"][k]) == n
                outputs[i] = {"tokens": out["sequences"][k][:n], "token_timestamps": out["token_timestamps"][k],
                              "stride": tuple(t / 16000 for t in windows[i][2])}
                mass[i], spread[i] = out["alignment_scores"][k], out["alignment_spreads"][k]
        order = sorted(outputs)
        assert order == list(range(len(windows)))
        _, words, groups = collate.decode_asr(vocab, [dict(outputs[i]) for i in order], return_timestamps="word", return_token_groups=True)
        want = R.word_scores(groups, np.concatenate([mass[i] for i in order]), np.concatenate([spread[i] for i in order]))
        assert [(w["alignment_score"], w["alignment_spread"]) for w in scored["chunks"]] == want
        # with the log-probabilities as well: independent of each other
        both = pipe(x, generate_kwargs=dict(gk), return_alignment_scores=True, return_scores=True)
        assert [{k: w[k] for k in ("text", "timestamp", "alignment_score", "alignment_spread")} for w in both["chunks"]] == scored["chunks"]
        assert all("logprob" in w for w in both["chunks"])
        with pytest.raises(ValueError, match="word"):
            pipe(x, generate_kwargs=dict(gk), return_timestamps=True, return_alignment_scores=True)

        # one window, one pass: forced alignment of the call's own tokens sees the same rows, so it returns the same values
        recorded.clear()
        y = syn.synth_audio(11, 20 * 16000, "mixed")
        free = pipe(y, generate_kwargs=dict(gk), return_alignment_scores=True, chunk_length_s=0)
        assert len(recorded) == 1
        out = recorded[0][1]
        ids = out["sequences"][0][:len(out["token_timestamps"][0])]
        if len(ids) == gk["max_new_tokens"]:
            # the decode ran into max_new_tokens: its last id was only predicted, never fed back, so it has no attention row of
            # its own; it takes the place of the eos in the forced rows (tests/test_gpu_align.py does the same)
            assert ids[-1] >= spec.timestamp_begin           # ... and here it is a timestamp token, part of no word
            ids = ids[:-1]
        forced = pipe.align(y, ids, language="<|en|>", task="transcribe", return_alignment_scores=True)
        assert forced["text"] == free["text"] and len(forced["chunks"]) == len(free["chunks"]) > 0
        for a, b in zip(forced["chunks"], free["chunks"]):
            assert a["text"] == b["text"] and np.isfinite(b["alignment_score"])
            assert a["alignment_score"] == b["alignment_score"] and a["alignment_spread"] == b["alignment_spread"]
    finally:
        monkeypatch.undo()
        pipe.engine.close()
