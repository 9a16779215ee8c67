"""Entropy of the teacher-forced positions (cw_set_score_entropy; the ENT forms of score_head_kernel / score_combine_kernel /
score_rows_kernel in csrc/score.hip) on the device: the head against float64 on its own f32 logits (the same operands through the
logits-storing form: the very accumulators) within the bound derived in tests/token_entropy_refs.py, and against float64 logits
rebuilt from the same 16-bit-rounded operands within that bound plus the first-order term at the rebuilt logits' own error bound;
the pre-existing outputs byte-identical with STOP and TOPK on; the row kernel on f32 logits with -inf / NaN columns and ldv > V; the
scoring calls with the switch on against off, fused head against loop path."""
import numpy as np
import pytest

import crisperwhisper_amd as cw
from crisperwhisper_amd import collate, synthetic as syn
from crisperwhisper_amd.engine import EngineError
from tests import helpers as Hh
from tests import test_gpu_score as SG
from tests import test_gpu_score_top as ST
from tests import token_entropy_refs as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


@pytest.fixture(scope="module")
def tiny():
    return Hh.tiny_setup()


def _n_split(M, V):
    """cw_score_head_splits (csrc/score.hip)."""
    NT, mt = (V + 15) // 16, (M + 127) // 128
    ns = max(1, min(256, 512 // mt))
    tps = ((NT + ns - 1) // ns + 3) & ~3
    return (NT + tps - 1) // tps


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("V", [250, 51866])
@pytest.mark.parametrize("M", [1, 127, 128, 129, 300])
def test_head_entropy(tiny, dtype, M, V):
    g_, v_, W, spec = tiny
    D = 128                                                       # the head's column walk does not depend on the width
    eng = ST._engine(spec, W, dtype, 2)
    try:
        x, g, b, emb, targets, ties = SG._head_case(dtype, M, D, V, 9000 + M + V)
        ns = _n_split(M, V)
        assert ns > 1
        depth = R.head_depth(V, ns)
        out = eng.test_score_head_entropy(x, g, b, emb, targets, want_logits=True)
        plain = eng.test_score_head(x, g, b, emb, targets)
        for key, ref in zip(("logprob", "top_id", "top_logprob"), plain):
            assert out[key].tobytes() == ref.tobytes()
        R.check_rows(out["entropy"], out["logits"], V, what=f"{dtype} M={M} V={V} own logits", depth=depth)
        # float64 logits from the same 16-bit operands; E: what the f32 accumulation and a LayerNorm rounding flip can move a logit by
        a16, flip = SG._ln16(x, g, b, dtype)
        w = emb.astype(np.float64)
        l64 = a16 @ w.T
        E = D * U * (np.abs(a16) @ np.abs(w).T) + (flip * np.abs(w).max(axis=0)[None, :]).sum(axis=1)[:, None]
        extra = [R.first_order(l64[m], V, float(E[m].max())) for m in range(M)]
        R.check_rows(out["entropy"], l64, V, what=f"{dtype} M={M} V={V} rebuilt logits", depth=depth, extra=extra)
        # joined with STOP and with TOPK: the same entropy bits, and every pre-existing output of those forms byte for byte
        stop = (V - 20, V - 10)
        k = 5
        s_on = eng.test_score_head_entropy(x, g, b, emb, targets, k=k, stop=stop)
        s_off = eng.test_score_head_top(x, g, b, emb, targets, k, stop=stop)
        assert s_on["entropy"].tobytes() == out["entropy"].tobytes()
        for key in ("logprob", "top_id", "top_logprob", "stop_logprob", "alt_id", "alt_logprob"):
            assert s_on[key].tobytes() == s_off[key].tobytes(), key
        t_on = eng.test_score_head_entropy(x, g, b, emb, targets, k=k)
        t_off = eng.test_score_head_top(x, g, b, emb, targets, k)
        assert t_on["entropy"].tobytes() == out["entropy"].tobytes()
        for key in ("logprob", "top_id", "top_logprob", "alt_id", "alt_logprob"):
            assert t_on[key].tobytes() == t_off[key].tobytes(), key
        p_on = eng.test_score_head_entropy(x, g, b, emb, targets, stop=stop)
        p_off = eng.test_score_head_stop(x, g, b, emb, targets, *stop)
        assert p_on["entropy"].tobytes() == out["entropy"].tobytes()
        for key, ref in zip(("logprob", "top_id", "top_logprob", "stop_logprob"), p_off):
            assert p_on[key].tobytes() == ref.tobytes(), key
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("V", [5, 250, 51866])
def test_rows_entropy(tiny, dtype, V):
    g_, v_, W, spec = tiny
    eng = ST._engine(spec, W, dtype, 2)
    try:
        rng = np.random.default_rng(V)
        rows, ldv = 9, V + 7
        lg = np.full((rows, ldv), 75.0, np.float32)               # ldv > V: what lies behind V must never count
        lg[:, :V] = rng.uniform(-60, 60, (rows, V))
        lg[1, :V][rng.random(V) < 0.5] = -np.inf; lg[1, 0] = 1.0
        lg[2, :V] = -np.inf; lg[2, V - 1] = 4.0                    # one finite logit: exactly 0
        lg[3, :V] = 0.25                                          # all equal: log V
        lg[4, V // 2] = np.nan
        lg[5, :V] = -np.inf                                       # F empty
        lg[6, V - 1] = np.inf
        targets = rng.integers(0, V, rows).astype(np.int32)
        out = eng.test_score_rows_entropy(lg, V, targets)
        ent = out["entropy"]
        assert ent[2] == 0.0 and np.isnan(ent[4]) and np.isnan(ent[5]) and np.isnan(ent[6])
        depth = ((V + 255) // 256, 6 + 4)                         # a thread adds ceil(V / 256) terms; 6 shuffle steps, 4 waves
        R.check_rows(ent, lg, V, what=f"{dtype} rows V={V}", depth=depth)
        assert abs(float(ent[3]) - np.log(V)) <= R.bound(lg[3], V, depth)
        stop = (max(0, V - 3), max(1, V - 2))
        both = eng.test_score_rows_entropy(lg, V, targets, k=4, stop=stop)
        ref = eng.test_score_rows_top(lg, V, targets, 4, stop=stop)
        assert both["entropy"].tobytes() == ent.tobytes()
        for key in ("logprob", "top_id", "top_logprob", "stop_logprob", "alt_id", "alt_logprob"):
            assert both[key].tobytes() == ref[key].tobytes(), key
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_engine_calls_on_against_off_and_head_against_loop(tiny, dtype):
    g, v, W, spec = tiny
    V = spec.vocab_size
    eng = ST._engine(spec, W, dtype, 9)
    try:
        n_rows = 9
        _, nf = eng.mel(ST._clips(n_rows))
        rows = ST._ragged_rows(v, spec, n_rows, 700 + n_rows, longest=False)
        off = eng.score_tokens(rows, 3)
        on = eng.score_tokens(rows, 3, entropy=True)
        both = eng.score_tokens(rows, 3, top_logprobs=4, entropy=True)
        top = eng.score_tokens(rows, 3, top_logprobs=4)
        assert len(on) == 4 and len(both) == 6
        for a, b_ in zip(off, on[:3]):
            ST._same_lists(a, b_)
        for a, b_ in zip(top, both[:5]):
            ST._same_lists(a, b_)
        ST._same_lists(on[3], both[5])
        for r in range(n_rows):
            assert len(on[3][r]) == len(rows[r]) - 3 and on[3][r].dtype == np.float32
            assert np.all(on[3][r] >= 0) and np.all(on[3][r] <= np.log(V) + 1e-4)
        a_on = eng.align_score_tokens(nf, rows, 3, entropy=True)
        a_off = eng.align_score_tokens(nf, rows, 3)
        for a, b_ in zip(a_off, a_on[:4]):
            ST._same_lists(a, b_)
        ST._same_lists(a_on[4], on[3])
        every = [np.ones(len(r) - 3, bool) for r in rows]
        forced = [r % 2 == 0 for r in range(n_rows)]
        c_off = eng.align_cut_tokens(nf, rows, 3, every, forced)
        c_on = eng.align_cut_tokens(nf, rows, 3, every, forced, entropy=True)
        assert np.array_equal(c_off[0], c_on[0]) and c_off[1].tobytes() == c_on[1].tobytes()
        for a, b_ in zip(c_off[2:], c_on[2:7]):
            ST._same_lists(a, b_)
        ST._same_lists(c_on[7], on[3])
        with pytest.raises(EngineError):
            eng.score_entropy(n_rows, max(len(r) for r in rows))              # off again after the call
        # the loop path: the step's f32 logits are captured, so its values are held against float64 on them; the fused head's
        # logits differ from those by the 16-bit forward's error, half of TOKEN_BOUND (a bound on a difference of two logits)
        eng.set_score_prefill(False)
        steps = max(len(r) for r in rows) - 3
        cap = eng.capture_logits(n_rows, steps)
        try:
            loop = eng.score_tokens(rows, 3, entropy=True)
            cap = cap.copy()
        finally:
            eng.stop_capture()
            eng.set_score_prefill(True)
        depth = ((V + 255) // 256, 6 + 4)
        worst = 0.0
        for r in range(n_rows):
            n = len(rows[r]) - 3
            R.check_rows(loop[3][r], cap[:n, r], V, what=f"{dtype} loop row {r}", depth=depth)
            if dtype != "f32":
                delta = SG.TOKEN_BOUND[dtype] / 2
                for j in range(n):
                    tol = R.first_order(cap[j, r], V, delta) + R.bound(cap[j, r], V, R.head_depth(V, 1)) + R.bound(cap[j, r], V, depth)
                    d = abs(float(on[3][r][j]) - float(loop[3][r][j]))
                    worst = max(worst, d / tol)
                    assert d <= tol, (r, j, d, tol)
            else:
                ST._same_lists(loop[3][r:r + 1], on[3][r:r + 1])              # the f32 engine has the loop path only
        print(dtype, "head vs loop: worst |difference| / tolerance =", worst)
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_teacher_forced_against_transformers(tiny, dtype):
    """transformers' teacher-forced forward over its own greedy sequences and the eos (tests/golden/gen_golden_token_entropy.py): every
    scored position, the eos's included, within the tolerance rule of tests/test_gpu_token_entropy.gold_tolerance -- the fused head
    on the 16-bit engines, the per-position loop on the f32 engine and, for bf16, on the loop path as well."""
    from tests.test_gpu_token_entropy import GOLD, _gold_clip, gold_tolerance
    g, v, W, spec = tiny
    eng = ST._engine(spec, W, dtype, 2)
    try:
        worst = 0.0
        for prefill in ((True, False) if dtype == "bf16" else (True,)):
            eng.set_score_prefill(prefill)
            for c in GOLD["cases"]:
                eng.mel([_gold_clip(c)])
                row = np.asarray(GOLD["init"] + c["ids"] + [GOLD["eos"]], np.int64)
                lp, ti, tl, en = eng.score_tokens([row], 3, entropy=True)
                ref = np.asarray(c["entropy"], np.float64)
                tol = gold_tolerance(c, dtype, len(ref))
                d = np.abs(en[0].astype(np.float64) - ref)
                worst = max(worst, float((d / tol).max()))
                assert len(en[0]) == len(ref) == len(c["ids"]) + 1 and np.all(d <= tol), (dtype, prefill, c["clip"], d.tolist(), tol.tolist())
        print(dtype, "teacher-forced worst |H - ref| / tolerance", worst)
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", ["bfloat16", "float32"])
def test_pipeline_score_align_align_long(tiny, dtype):
    """return_entropy on score / align / align_long: the result keys, the values being the engine's arrays, and everything else in
    the result being what the call without it returns."""
    g, v, W, spec = tiny
    pipe = cw.pipeline("automatic-speech-recognition", model=cw.ModelBundle(spec, W), tokenizer=collate.Vocabulary.from_synthetic(v),
                       batch_size=4, return_timestamps="word", torch_dtype=dtype, device="cuda:0")
    drop = lambda d, keys: {k_: x for k_, x in d.items() if k_ not in keys}
    word_keys = ("entropy", "entropy_max")

    def check_words(chunks, logV):
        for c in chunks:
            assert isinstance(c["entropy"], float) and 0 <= c["entropy"] <= c["entropy_max"] <= logV + 1e-4
            if "tokens" in c:
                h = np.asarray([t["entropy"] for t in c["tokens"]], np.float64)
                assert c["entropy"] == float(np.mean(h)) and c["entropy_max"] == float(np.max(h))
    try:
        kw = dict(language="<|en|>", task="transcribe")
        logV = float(np.log(spec.vocab_size))
        short = syn.synth_audio(90, 16000 * 4, "mixed")
        text = [ord(c) for c in " abc def ghi"]
        plain = pipe.score(short, text, **kw)
        assert pipe.score(short, text, return_entropy=False, **kw) == plain
        sc = pipe.score(short, text, return_entropy=True, **kw)
        assert set(sc) == set(plain) | {"avg_entropy"}
        assert drop(sc, ("avg_entropy", "tokens", "chunks")) == drop(plain, ("tokens", "chunks"))
        assert [drop(t, ("entropy",)) for t in sc["tokens"]] == plain["tokens"]
        assert [drop(c, word_keys) for c in sc["chunks"]] == plain["chunks"]
        eng = pipe.engine
        eng.mel([short])
        row = np.asarray([v.sot, v.lang_id("en"), v.transcribe] + text + [v.eos], np.int64)
        en = eng.score_tokens([row], 3, entropy=True)[3][0].astype(np.float64)
        assert [t["entropy"] for t in sc["tokens"]] == en.tolist() and sc["avg_entropy"] == float(en.mean())
        check_words(sc["chunks"], logV)
        assert [c["entropy_max"] for c in sc["chunks"]] == [float(en[4 * i:4 * i + 4].max()) for i in range(3)]   # " abc": 4 tokens a word
        both = pipe.score(short, text, return_entropy=True, top_logprobs=3, **kw)
        assert [t["entropy"] for t in both["tokens"]] == en.tolist() and all("rank" in t for t in both["tokens"])

        a_plain = pipe.align(short, text, return_scores=True, **kw)
        assert pipe.align(short, text, return_scores=True, return_entropy=False, **kw) == a_plain
        a_en = pipe.align(short, text, return_scores=True, return_entropy=True, top_logprobs=2, **kw)
        assert set(a_en) == set(a_plain) | {"avg_entropy"} and a_en["avg_entropy"] == sc["avg_entropy"]
        assert [drop(c, word_keys + ("tokens",)) for c in a_en["chunks"]] == a_plain["chunks"]
        check_words(a_en["chunks"], logV)
        assert [t["entropy"] for c in a_en["chunks"] for t in c["tokens"]] == en[:-1].tolist()
        a_only = pipe.align(short, text, return_scores=True, return_entropy=True, **kw)
        assert [drop(c, word_keys) for c in a_only["chunks"]] == a_plain["chunks"]
        assert [[c[k_] for k_ in word_keys] for c in a_only["chunks"]] == [[c[k_] for k_ in word_keys] for c in a_en["chunks"]]

        long_clip = syn.synth_audio(7, 16000 * 70, "mixed")
        ltext = [ord(c) for c in " abc" * 15]
        l_plain = pipe.align_long(long_clip, ltext, return_scores=True, max_window_tokens=16, **kw)
        assert pipe.align_long(long_clip, ltext, return_scores=True, return_entropy=False, max_window_tokens=16, **kw) == l_plain
        l_en = pipe.align_long(long_clip, ltext, return_scores=True, return_entropy=True, top_logprobs=2, max_window_tokens=16, **kw)
        assert len(pipe.stats["align_long"]) >= 3
        assert set(l_en) == set(l_plain) | {"avg_entropy"} and drop(l_en, ("avg_entropy", "chunks")) == drop(l_plain, ("chunks",))
        assert [drop(c, word_keys + ("tokens",)) for c in l_en["chunks"]] == l_plain["chunks"]
        check_words(l_en["chunks"], logV)
        flat = [t for c in l_en["chunks"] for t in c["tokens"]]
        assert [t["id"] for t in flat] == ltext and 0 <= l_en["avg_entropy"] <= logV + 1e-4
        for fn, args in ((pipe.align, (short, text)), (pipe.align_long, (long_clip, ltext))):
            with pytest.raises(ValueError, match="return_scores"):
                fn(*args, return_entropy=True, **kw)                          # needs return_scores=True
    finally:
        pipe.engine.close()
