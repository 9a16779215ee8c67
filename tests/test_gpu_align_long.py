"""Long-form forced alignment on the device (score.hip STOP forms, align.hip align_cut_kernel, cw_align_cut_tokens,
Engine.align_cut_tokens, CrisperWhisperPipeline.align_long).

* The STOP head (cw_test_score_head_stop) against float64, with the stop set S = {eos} + {n >= tb} placed in the last tile only,
  split between the first tile and the tail, reduced to {eos}, holding the row's +60 maximum, and >= 100 nats under the row's
  maximum; its other three outputs bit-identical to the plain head's.
* The cut kernel (cw_test_align_cut) against the float64 restatement of tests/align_long_refs.py: equal cuts, bit-equal scores.
* cw_align_cut_tokens on all three engines: cut / cut_score are the restatement of the call's own scores; scores bit-identical to
  align_score_tokens; timestamps those of align_tokens on the kept prefix; prefill against the loop; stop_logprob against
  float64 of the f32 engine's logits.
* align_long against align (audio <= 30 s), against a walk written here (70 s), lists against single recordings, refusals.

Error bound of the head test: test_gpu_score.py's docstring derives E (per logit: D u A + F) and the error of a float32
logsumexp over the row, (V / 16 + 400) u + 4 u (1 + |lse|) beyond E_row.  stop_logprob = lse_S - lse is the difference of two such
reductions, the first over S alone (its logits move by at most max_{n in S} E[n], its sum has no more terms than the row's):
  |err| <= max_{n in S} E[n] + E_row + 2 (V / 16 + 400) u + 4 u (1 + |lse| + |lse_S|).
"""
import ctypes as C

import numpy as np
import pytest

import crisperwhisper_amd as cw
from crisperwhisper_amd import collate, synthetic as syn
from crisperwhisper_amd.engine import Engine, EngineError
from tests import align_long_refs as R
from tests import helpers as Hh
from tests.test_gpu_score import TOKEN_BOUND, U, _head_case, _ln16, _round16

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tiny():
    return Hh.tiny_setup()


def _engine(spec, W, dtype, rows=8):
    e = Engine(spec, dtype=dtype, max_batch=rows)
    e.load_state_dict(W)
    return e


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------ head
def _head_reference(dtype, x, g, b, emb):
    M, D = x.shape
    V = emb.shape[0]
    a16, flip = _ln16(x, g, b, dtype)
    w = emb.astype(np.float64)
    F = (flip * np.abs(w).max(axis=0)[None, :]).sum(axis=1)
    l64 = np.empty((M, V)); E = np.empty((M, V))
    for n0 in range(0, V, 8192):
        ws = w[n0:n0 + 8192]
        l64[:, n0:n0 + 8192] = a16 @ ws.T
        E[:, n0:n0 + 8192] = D * U * (np.abs(a16) @ np.abs(ws).T) + F[:, None]
    return l64, E


def _lse_rows(l):
    m = l.max(axis=1)
    return m + np.log(np.exp(l - m[:, None]).sum(axis=1))


def _check_stop(eng, dtype, x, g, b, emb, targets, l64, E, eos, tb, plain):
    V = emb.shape[0]
    lp, ti, tl, sl = eng.test_score_head_stop(x, g, b, emb, targets, eos, tb)
    assert np.array_equal(_bits(lp), _bits(plain[0])) and np.array_equal(ti, plain[1]) and np.array_equal(_bits(tl), _bits(plain[2]))
    S = R.stop_set(V, eos, tb)
    lse, lse_s = _lse_rows(l64), _lse_rows(l64[:, S])
    bound = E[:, S].max(axis=1) + E.max(axis=1) + 2 * (V / 16 + 400) * U + 4 * U * (1 + np.abs(lse) + np.abs(lse_s))
    err = np.abs(sl.astype(np.float64) - (lse_s - lse))
    print(dtype, x.shape[0], V, "eos", eos, "tb", tb, "worst err / bound", float((err / bound).max()), "min stop", float(sl.min()))
    assert np.isfinite(sl).all()
    assert np.all(err <= bound), (dtype, eos, tb, int(np.argmax(err - bound)), float(err.max()), float(bound.min()))
    assert np.all(sl.astype(np.float64) <= bound)                      # a log-probability: never above 0 by more than the bound
    return sl, lse_s - lse


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("V", [48, 250])
@pytest.mark.parametrize("M", [1, 37, 130])
def test_stop_head_vs_float64(tiny, dtype, M, V):
    g_, v_, W, spec = tiny
    x, g, b, emb, targets, ties = _head_case(dtype, M, 128, V, 7000 + M + V)
    hi, lo = V // 2, V // 2 + 1
    if M == 1:                                                         # _head_case plants +-60 from two rows on: a -80 for row 0
        a16, _ = _ln16(x, g, b, dtype)
        emb[lo] = _round16((-a16[0] / np.dot(a16[0], a16[0]) * 80.0).astype(np.float32), dtype)
    l64, E = _head_reference(dtype, x, g, b, emb)
    eng = _engine(spec, W, dtype, rows=2)
    try:
        plain = eng.test_score_head(x, g, b, emb, targets)
        args = (eng, dtype, x, g, b, emb, targets, l64, E)
        _check_stop(*args, V - 2, V - 1, plain)                        # S inside the last tile only
        _check_stop(*args, 2, V - 3, plain)                            # eos in the first tile, the timestamps at the tail
        _check_stop(*args, 5, V, plain)                                # tb = V: S = {eos}
        m = M - 1
        top = hi if M > 1 else V - 1                                   # the row's planted maximum (+60; row 0: +30 at V - 1)
        sl, want = _check_stop(*args, top, V - 3, plain)               # S holds the maximum of row m
        assert int(np.argmax(l64[m])) == top and want[m] > -1e-3 and sl[m] > -1e-2
        sl, want = _check_stop(*args, lo, V, plain)                    # S = {lo}: >= 100 nats under the maximum of row m
        assert l64[m].max() - l64[m, lo] >= 100 and want[m] <= -100 and np.isfinite(sl[m])
    finally:
        eng.close()


def test_stop_head_full_vocabulary(tiny):
    g_, v_, W, spec = tiny
    dtype = "bf16"
    x, g, b, emb, targets, ties = _head_case(dtype, 64, 1280, 51866, 99)
    l64, E = _head_reference(dtype, x, g, b, emb)
    eng = _engine(spec, W, dtype, rows=2)
    try:
        plain = eng.test_score_head(x, g, b, emb, targets)
        _check_stop(eng, dtype, x, g, b, emb, targets, l64, E, 50257, 50365, plain)
    finally:
        eng.close()


def test_stop_head_refuses_bad_arguments(tiny):
    g_, v_, W, spec = tiny
    eng = _engine(spec, W, "bf16", rows=2)
    try:
        x = np.zeros((2, 64), np.float32); emb = np.zeros((20, 64), np.float32); one = np.ones(64, np.float32)
        for eos, tb in ((20, 20), (-1, 5), (3, 21), (3, -1)):
            with pytest.raises(EngineError):
                eng.test_score_head_stop(x, one, one, emb, [0, 1], eos, tb)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------------- cut
N_CHOICES = (0, 1, 2, 63, 64, 65, 444)


def _cut_rows(n_rows, seed):
    rng = np.random.default_rng(seed)
    Ns = [N_CHOICES[(k + seed) % len(N_CHOICES)] for k in range(n_rows)]
    lp = [(-rng.exponential(3.0, N + 1)).astype(np.float32) for N in Ns]
    st = [(-rng.exponential(5.0, N + 1)).astype(np.float32) for N in Ns]
    return Ns, lp, st


def _check_cut(eng, lp, st, masks, force):
    cut, score = eng.test_align_cut(lp, st, masks, force)
    for r in range(len(lp)):
        want, ws = R.cut(lp[r], st[r], masks[r], force[r])
        assert cut[r] == want, (r, len(lp[r]) - 1, int(cut[r]), want)
        assert _bits(score[r:r + 1])[0] == _bits(np.array([ws]))[0], (r, float(score[r]), float(ws))
    return cut, score


@pytest.mark.parametrize("n_rows", [1, 9, 64])
def test_cut_kernel_vs_float64(tiny, n_rows):
    g_, v_, W, spec = tiny
    eng = _engine(spec, W, "f32", rows=2)
    try:
        for seed in range(7 if n_rows == 1 else 2):                    # one row: every N of the list
            Ns, lp, st = _cut_rows(n_rows, seed)
            none = [False] * n_rows
            first = [np.arange(N + 1) == 0 for N in Ns]
            last = [np.arange(N + 1) == N for N in Ns]
            third = [np.arange(N + 1) % 3 == 0 for N in Ns]
            every = [np.ones(N + 1, bool) for N in Ns]
            cut, _ = _check_cut(eng, lp, st, first, none)
            assert cut.tolist() == [0] * n_rows
            cut, _ = _check_cut(eng, lp, st, last, none)
            assert cut.tolist() == Ns
            _check_cut(eng, lp, st, third, none)
            _check_cut(eng, lp, st, every, none)
            # -inf stop entries, on allowed candidates too
            rng = np.random.default_rng(50 + seed)
            st_inf = [s.copy() for s in st]
            for s in st_inf:
                s[rng.random(s.size) < 0.5] = -np.inf
            _check_cut(eng, lp, st_inf, every, none)
            _check_cut(eng, lp, [np.full_like(s, -np.inf) for s in st], third, none)      # all tie at -inf: the first allowed
            # forced rows, the mask all zero; mixed with unforced ones
            zero = [np.zeros(N + 1, bool) for N in Ns]
            cut, _ = _check_cut(eng, lp, st, zero, [True] * n_rows)
            assert cut.tolist() == Ns
            mixed = [r % 2 == 0 for r in range(n_rows)]
            _check_cut(eng, lp, st, [z if f else e for z, e, f in zip(zero, every, mixed)], mixed)
            # planted exact ties: lp = -1 throughout, so S[n] = -n + st[n]; st[b] = st[a] + (b - a) makes S[a] == S[b]
            lp1 = [np.full(N + 1, -1.0, np.float32) for N in Ns]
            st_t, lows = [], []
            for N in Ns:
                s = np.full(N + 1, -3000.0, np.float32)
                a, b_ = (N // 3, N) if N >= 1 else (0, 0)
                s[a] = -1000.0
                s[b_] = -1000.0 + (b_ - a)
                st_t.append(s); lows.append(a)
            cut, score = _check_cut(eng, lp1, st_t, every, none)
            assert cut.tolist() == lows
            assert all(R.prefix_scores(l, s)[a] == R.prefix_scores(l, s)[len(l) - 1] for l, s, a in zip(lp1, st_t, lows))
        with pytest.raises(EngineError, match="allows no cut"):
            eng.test_align_cut(lp, st, zero, [r != n_rows - 1 for r in range(n_rows)])     # one unforced all-zero row
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------- engine
def _rows(v, spec, n_rows, seed, longest=False):
    rng = np.random.default_rng(seed)
    init = [v.sot, v.lang_id("en"), v.transcribe]
    lens = rng.integers(3, 40, n_rows)
    lens[0] = 3
    if longest and n_rows > 1:
        lens[1] = spec.max_target_positions - len(init) - 1
    return [np.asarray(init + rng.integers(0, 256, n).tolist() + [v.eos], np.int64) for n in lens]


def _clips(n, seed=150):
    return [syn.synth_audio(seed + k, 16000 * (4 if k % 2 else 30), ("mixed", "noise", "chirp")[k % 3]) for k in range(n)]


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_align_cut_tokens_engine(tiny, dtype):
    g, v, W, spec = tiny
    eng = _engine(spec, W, dtype, rows=9)
    try:
        for n_rows in (1, 8, 9):
            _, nf = eng.mel(_clips(n_rows))
            rows = _rows(v, spec, n_rows, 400 + n_rows, longest=(dtype != "f32" and n_rows == 8))
            Ns = [len(r) - 4 for r in rows]
            rng = np.random.default_rng(n_rows)
            interior = [int(rng.integers(1, N)) for N in Ns]           # exactly one n strictly between 0 and N
            masks = [np.arange(N + 1) == k for N, k in zip(Ns, interior)]
            none = [False] * n_rows
            cut, score, ts, lp, sl, ti, tl = eng.align_cut_tokens(nf, rows, 3, masks, none)
            assert cut.tolist() == interior
            ts2, lp2, ti2, tl2 = eng.align_score_tokens(nf, rows, 3)
            pre = eng.align_tokens(nf, [np.concatenate([r[:3 + c], [v.eos]]) for r, c in zip(rows, cut)], 3)
            for r in range(n_rows):
                want, ws = R.cut(lp[r], sl[r], masks[r], False)
                assert cut[r] == want and _bits(score[r:r + 1])[0] == _bits(np.array([ws]))[0]
                assert np.array_equal(_bits(lp[r]), _bits(lp2[r])) and np.array_equal(ti[r], ti2[r])
                assert np.array_equal(_bits(tl[r]), _bits(tl2[r]))
                assert np.isfinite(sl[r]).all() and np.all(sl[r] <= 1e-5) and len(sl[r]) == Ns[r] + 1
                assert len(ts[r]) == 3 + cut[r] + 1 == len(pre[r])
                assert np.array_equal(_bits(ts[r]), _bits(pre[r])), (dtype, n_rows, r, ts[r].tolist(), pre[r].tolist())
            # forced rows take everything and give align_score_tokens' timestamps; a free choice is the restatement's
            forced = [r % 2 == 0 for r in range(n_rows)]
            every = [np.ones(N + 1, bool) for N in Ns]
            cut, score, ts, lp, sl, ti, tl = eng.align_cut_tokens(nf, rows, 3, every, forced)
            for r in range(n_rows):
                want, ws = R.cut(lp[r], sl[r], every[r], forced[r])
                assert cut[r] == want and _bits(score[r:r + 1])[0] == _bits(np.array([ws]))[0]
                if forced[r]:
                    assert cut[r] == Ns[r] and np.array_equal(_bits(ts[r]), _bits(ts2[r]))
            print(dtype, n_rows, "rows: free cuts", cut.tolist(), "of", Ns)
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_prefill_and_loop_choose_the_same_cut(tiny, dtype):
    """Two candidates per row, a and a + max(2, N // 2) tokens: the scores of the two forwards differ by at most TOKEN_BOUND per
    token, so S differs by at most TOKEN_BOUND (N + 1); where the winner leads the runner-up by more than twice that in both
    score sets the cuts must agree.  The f32 engine has one forward: no row is skipped there."""
    g, v, W, spec = tiny
    eng = _engine(spec, W, dtype, rows=9)
    try:
        skipped = total = 0
        for n_rows in (1, 8, 9):
            _, nf = eng.mel(_clips(n_rows))
            rows = _rows(v, spec, n_rows, 500 + n_rows)
            Ns = [len(r) - 4 for r in rows]
            rng = np.random.default_rng(n_rows)
            masks = []
            for N in Ns:
                a = int(rng.integers(0, N - max(2, N // 2) + 1))
                m = np.zeros(N + 1, bool); m[a] = m[a + max(2, N // 2)] = True
                masks.append(m)
            none = [False] * n_rows
            eng.set_score_prefill(True)
            c1, s1, _, lp1, sl1, _, _ = eng.align_cut_tokens(nf, rows, 3, masks, none)
            eng.set_score_prefill(False)
            c2, s2, _, lp2, sl2, _, _ = eng.align_cut_tokens(nf, rows, 3, masks, none)
            eng.set_score_prefill(True)
            for r in range(n_rows):
                total += 1
                if dtype == "f32":
                    assert c1[r] == c2[r] and _bits(s1[r:r + 1])[0] == _bits(s2[r:r + 1])[0]
                    continue
                assert np.abs(sl1[r] - sl2[r]).max() <= TOKEN_BOUND[dtype], (r, float(np.abs(sl1[r] - sl2[r]).max()))
                margin = 2 * TOKEN_BOUND[dtype] * (Ns[r] + 1)
                gaps = [abs(float(np.diff(R.prefix_scores(l, s)[masks[r]])[0])) for l, s in ((lp1[r], sl1[r]), (lp2[r], sl2[r]))]
                if min(gaps) <= margin:
                    skipped += 1
                    continue
                assert c1[r] == c2[r], (dtype, n_rows, r, int(c1[r]), int(c2[r]), gaps, margin)
        print(dtype, "rows skipped as too close:", skipped, "of", total)
        assert skipped <= 0.2 * total
    finally:
        eng.close()


def test_stop_logprob_against_float64_of_the_logits(tiny):
    """f32 engine: stop_logprob within 4e-3 (the engine's per-token bound) of the float64 value of the logits the decode loop
    exposes through its capture; the 16-bit engines within TOKEN_BOUND of the f32 engine."""
    g, v, W, spec = tiny
    clips = _clips(3)
    rows = _rows(v, spec, 3, 77)
    Ns = [len(r) - 4 for r in rows]
    every = [np.ones(N + 1, bool) for N in Ns]
    eos, tb = spec.eos_token_id, spec.timestamp_begin
    ref = None
    for dtype in ("f32", "bf16", "f16"):
        eng = _engine(spec, W, dtype, rows=4)
        try:
            _, nf = eng.mel(clips)
            if dtype == "f32":
                cap = eng.capture_logits(3, max(Ns) + 1)
                out = eng.align_cut_tokens(nf, rows, 3, every, [False] * 3)
                cap = np.array(cap, copy=True)
                eng.stop_capture()
                ref = out[4]
                for r in range(3):
                    want = R.stop_logprob(cap[:Ns[r] + 1, r], eos, tb)
                    err = np.abs(ref[r].astype(np.float64) - want)
                    print("f32 row", r, "worst |stop - float64| =", float(err.max()))
                    assert err.max() <= 4e-3
            else:
                sl = eng.align_cut_tokens(nf, rows, 3, every, [False] * 3)[4]
                for r in range(3):
                    assert np.abs(sl[r] - ref[r]).max() <= TOKEN_BOUND[dtype]
        finally:
            eng.close()


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_engine_refusals_before_a_launch(tiny, dtype):
    g, v, W, spec = tiny
    eng = _engine(spec, W, dtype, rows=4)
    try:
        _, nf = eng.mel(_clips(2))
        init = [v.sot, v.lang_id("en"), v.transcribe]
        good = np.asarray(init + [5, 6, 7, v.eos], np.int64)
        runs = eng.score_prefill_runs()
        with pytest.raises(EngineError, match="allows no cut"):
            eng.align_cut_tokens(nf[:1], [good], 3, [np.zeros(4, bool)], [False])
        with pytest.raises(EngineError):
            eng.align_cut_tokens(nf[:1], [np.asarray(init + [5, v.eos, 6, v.eos])], 3, [np.ones(4, bool)], [False])   # eos inside
        with pytest.raises(ValueError):
            eng.align_cut_tokens(nf[:1], [good], 3, [np.ones(3, bool)], [False])                 # N flags instead of N + 1
        tab = np.ascontiguousarray(good[None].astype(np.int32)); n = np.asarray([len(good)], np.int32)
        nf1 = np.asarray(nf[:1], np.int32); ok = np.ones((1, 7), np.uint8); fo = np.zeros(1, np.uint8)
        P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        outs = [np.zeros(1, np.int32), np.zeros(1, np.float32), np.zeros(7, np.float32), np.zeros(7, np.float32), np.zeros(7, np.float32)]
        for drop in range(7):                                          # cut_ok, force_all and the five required outputs
            a = [ok, fo] + outs
            a[drop] = None
            rc = eng.lib.cw_align_cut_tokens(eng.ctx, 1, P(nf1), P(tab), 7, P(n), 3, *[P(x) for x in a], None, None)
            assert rc != 0 and "null argument" in eng.lib.cw_last_error(eng.ctx).decode()
        assert eng.score_prefill_runs() == runs
        cut = eng.align_cut_tokens(nf[:1], [good], 3, [np.ones(4, bool)], [True])[0]             # and the context still works
        assert cut.tolist() == [3]
    finally:
        eng.close()


# -------------------------------------------------------------------------------------------------------------- pipeline
def _pipe(tiny, dtype, batch=4):
    g, v, W, spec = tiny
    return cw.pipeline("automatic-speech-recognition", model=cw.ModelBundle(spec, W), tokenizer=collate.Vocabulary.from_synthetic(v),
                       batch_size=batch, return_timestamps="word", torch_dtype=dtype, device="cuda:0")


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_align_long_is_align_up_to_thirty_seconds(tiny, dtype):
    pipe = _pipe(tiny, dtype)
    try:
        clips = [syn.synth_audio(90, 16000 * 30, "mixed"), syn.synth_audio(91, 16000 * 4, "noise"), syn.synth_audio(92, 16000 * 12, "chirp")]
        texts = [[ord(c) for c in t] for t in (" abc def ghi jkl", " hello, world", " a")]
        kw = dict(language="<|en|>", task="transcribe")
        for opts in ({}, {"return_scores": True}, {"return_alignment_scores": True},
                     {"return_scores": True, "return_alignment_scores": True, "alignment_collar_frames": 2}):
            want = pipe.align(clips, texts, **kw, **opts)
            got = pipe.align_long(clips, texts, **kw, **opts)
            assert len(got) == 3
            for gk, wk in zip(got, want):
                assert gk["text"] == wk["text"] and set(gk) == set(wk)
                assert len(gk["chunks"]) == len(wk["chunks"])
                for a, b in zip(gk["chunks"], wk["chunks"]):
                    assert set(a) == set(b) and a["text"] == b["text"] and tuple(a["timestamp"]) == tuple(b["timestamp"])
                    for key in set(a) - {"text", "timestamp"}:
                        assert a[key] == b[key] or (a[key] != a[key] and b[key] != b[key]), (key, a, b)
                for key in set(gk) - {"text", "chunks"}:
                    assert gk[key] == wk[key], (key, gk[key], wk[key])
            assert [(t["item"], t["forced"], t["seek_s"]) for t in pipe.stats["align_long"]] == [(0, True, 0.0), (1, True, 0.0), (2, True, 0.0)]
        one = pipe.align_long(clips[1], texts[1], **kw)
        assert isinstance(one, dict) and one["text"] == " hello, world"
    finally:
        pipe.engine.close()


def _reference_walk(pipe, v, pcm, T, cap):
    """align_long restated from Engine.align_cut_tokens for the cut and the scores, Engine.align_tokens on every kept prefix for
    the timestamps, and the collator."""
    eng, spec, vocab = pipe.engine, pipe.bundle.spec, pipe.vocab
    v_init = [v.sot, v.lang_id("en"), v.transcribe]
    T = np.asarray(T, np.int64)
    N, WIN = len(T), 480000
    _, _, groups = collate.decode_asr(vocab, [{"tokens": T, "token_timestamps": np.zeros(N, np.float32)}], time_precision=0.02,
                                      return_timestamps="word", return_token_groups=True)
    bounds = sorted({min(g_) for g_ in groups} | {N})
    pos = seek = 0
    chunks, cuts = [], []
    while pos < N:
        _, nf = eng.mel([pcm[seek:seek + WIN]])
        last = seek + WIN >= len(pcm)
        L = max(x for x in bounds if pos < x <= pos + min(N - pos, cap)) - pos
        ok = np.array([(pos + n in bounds) or n == 0 for n in range(L + 1)])
        row = np.concatenate([v_init, T[pos:pos + L], [spec.eos_token_id]])
        cut = int(eng.align_cut_tokens(nf, [row], 3, [ok], [last])[0][0])
        cuts.append((seek, L, cut, last))
        if cut:
            ts = eng.align_tokens(nf, [np.concatenate([v_init, T[pos:pos + cut], [spec.eos_token_id]])], 3)[0]
            _, words = collate.decode_asr(vocab, [{"tokens": T[pos:pos + cut], "token_timestamps": ts[3:3 + cut]}],
                                          time_precision=0.02, return_timestamps="word")
            end = words[-1]["timestamp"][1]
            chunks += [{"text": w["text"], "timestamp": tuple(round(t + seek / 16000, 2) for t in w["timestamp"])} for w in words]
            pos += cut
            if not last:
                seek += (int(round(end * 100)) // 2) * 320
        elif not last:
            seek += WIN
    return chunks, cuts


def test_align_long_seventy_seconds_against_a_reference_walk(tiny):
    pipe = _pipe(tiny, "float32")
    try:
        pcm70, pcm41 = syn.synth_audio(7, 16000 * 70, "mixed"), syn.synth_audio(8, 16000 * 41, "chirp")
        T = [ord(c) for c in " abc" * 15]                              # 60 tokens, 15 words
        T2 = [ord(c) for c in " de fgh" * 4]
        kw = dict(language="<|en|>", task="transcribe")
        for cap in (16, None):
            got = pipe.align_long(pcm70, T, max_window_tokens=cap, **kw)
            trace = list(pipe.stats["align_long"])
            want, cuts = _reference_walk(pipe, tiny[1], pcm70, T, cap if cap else tiny[3].max_target_positions - 4)
            print("max_window_tokens", cap, "(seek, offered, cut, forced):", cuts)
            assert got["text"] == " abc" * 15
            assert [(c["text"], tuple(c["timestamp"])) for c in got["chunks"]] == [(c["text"], c["timestamp"]) for c in want]
            assert [(int(round(t["seek_s"] * 16000)), t["offered"], t["cut"], t["forced"]) for t in trace] == cuts
            assert cuts[-1][3] and sum(c[2] for c in cuts) == 60
        both = pipe.align_long([pcm70, pcm41], [T, T2], return_scores=True, max_window_tokens=16, **kw)
        for k, (x, t) in enumerate(((pcm70, T), (pcm41, T2))):
            alone = pipe.align_long(x, t, return_scores=True, max_window_tokens=16, **kw)
            assert both[k]["text"] == alone["text"]
            assert [(c["text"], tuple(c["timestamp"])) for c in both[k]["chunks"]] == [(c["text"], tuple(c["timestamp"])) for c in alone["chunks"]]
            # (the f32 decode step picks kernels by batch size: scores agree within its bound, not bit for bit)
            assert both[k]["logprob"] == pytest.approx(alone["logprob"], abs=4e-3 * (len(t) + 1))
    finally:
        pipe.engine.close()


def test_align_long_refusals_before_a_launch(tiny):
    g, v, W, spec = tiny
    pipe = _pipe(tiny, "bfloat16")
    try:
        x = syn.synth_audio(3, 16000 * 40, "noise")
        runs = pipe.engine.score_prefill_runs()
        kw = dict(language="<|en|>", task="transcribe")
        with pytest.raises(ValueError, match="timestamp token"):
            pipe.align_long(x, [32, 97, v.timestamp_begin + 1], **kw)
        with pytest.raises(ValueError, match="above the 2"):
            pipe.align_long(x, [32, 97, 98], max_window_tokens=2, **kw)
        with pytest.raises(ValueError, match="2 transcripts"):
            pipe.align_long([x, x], [[32, 97]], **kw)
        with pytest.raises(ValueError):
            pipe.align_long(x, [32, 97], language="<|xx|>")
        assert pipe.align_long(x, [], **kw) == {"text": "", "chunks": []}
        assert pipe.engine.score_prefill_runs() == runs
        with pytest.raises(ValueError, match="30 s"):                  # align keeps its refusal, and points here
            pipe.align(x, [32, 97], **kw)
        out = pipe.align_long(x, [32, 97, 32, 98], **kw)
        assert out["text"] == " a b" and pipe.engine.score_prefill_runs() > runs
    finally:
        pipe.engine.close()
