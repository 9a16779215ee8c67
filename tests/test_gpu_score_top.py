"""Alternatives of teacher-forced positions on the device (score.hip TOPK forms, cw_set_score_top_logprobs,
Engine.score_tokens / align_score_tokens / align_cut_tokens(top_logprobs=k), CrisperWhisperPipeline.score / align / align_long).

* The fused head (cw_test_score_head_top) against its own logits: the hook runs the same operands through the head's
  logits-storing form as well -- the same MFMA sequence, so the very f32 numbers the fused form selected from.  Ids must equal the
  (value descending, id ascending) sort of those logits exactly; values lie within the sum-and-subtraction bound of
  tests/score_top_refs.py.  Bit identities: rank 0 is top_id / top_logprob, the target's entry is token_logprob, and everything
  the plain head returns is returned unchanged.  The hook's device arrays carry guard rows behind row M - 1.
* Planted rows: the cases the list / threshold / merge scheme can get wrong (one lane's columns, one best per split, the last
  split next to the padding columns, no insertion after the fill, every column inserting, exact ties across and inside splits).
* The STOP form, the row kernel of the loop path on caller-supplied logits (NaN, -inf, pad columns, ties), the engine calls on
  all three engines (k = 8 against k = 0 bit for bit; prefill against loop; rows_per_item), the pipeline.

A row that holds a NaN has a NaN normaliser today (token_logprob is NaN there); its alternatives keep their ids and hold NaN.
A row without any candidate lists -1 / NaN at rank 0, where top_id holds its own "none" value.
"""
import numpy as np
import pytest

import crisperwhisper_amd as cw
from crisperwhisper_amd import collate, synthetic as syn
from crisperwhisper_amd.engine import Engine, EngineError
from tests import helpers as Hh
from tests import score_top_refs as R
from tests.test_gpu_score import TOKEN_BOUND, _clips, _head_case, _ln16, _ragged_rows, _round16

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def tiny():
    return Hh.tiny_setup()


@pytest.fixture(scope="module")
def engines(tiny):
    g, v, W, spec = tiny
    made = {}

    def get(dtype):
        if dtype not in made:
            made[dtype] = Engine(spec, dtype=dtype, max_batch=2)
            made[dtype].load_state_dict(W)
        return made[dtype]
    yield get
    for e in made.values():
        e.close()


def _identities(out, plain, targets, k):
    """The contract's bit identities of one head / row-kernel result; plain = (logprob, top_id, top_logprob[, stop]) of k = 0."""
    ids, lp = out["alt_id"], out["alt_logprob"]
    some = ids[:, 0] >= 0
    assert np.array_equal(ids[some, 0], out["top_id"][some])
    assert np.array_equal(_bits(lp[some, 0]), _bits(out["top_logprob"][some]))
    hit = ids[:, :k] == np.asarray(targets)[:, None]
    rows, ranks = np.nonzero(hit)
    assert np.array_equal(_bits(lp[rows, ranks]), _bits(out["logprob"][rows]))
    if plain is not None:
        assert np.array_equal(_bits(plain[0]), _bits(out["logprob"])) and np.array_equal(plain[1], out["top_id"])
        assert np.array_equal(_bits(plain[2]), _bits(out["top_logprob"]))
        if len(plain) > 3:
            assert np.array_equal(_bits(plain[3]), _bits(out["stop_logprob"]))
    return int(hit.any(axis=1).sum())


def _check_head_top(eng, x, g, b, emb, targets, k, stop=None):
    V = emb.shape[0]
    out = eng.test_score_head_top(x, g, b, emb, targets, k, want_logits=True, stop=stop)
    z = out["logits"]
    problems, worst = R.check_topk(out["alt_id"], out["alt_logprob"], z, V, k, V / 16, R.HEAD_C)
    assert not problems, problems[:3]
    plain = eng.test_score_head(x, g, b, emb, targets) if stop is None else eng.test_score_head_stop(x, g, b, emb, targets, *stop)
    n_hit = _identities(out, plain, targets, k)
    return out, z, worst, n_hit


# ------------------------------------------------------------------------------------------------------------------ head
HEAD_SHAPES = [(M, V) for M in (1, 37, 130) for V in (5, 48, 250)] + [(37, 51866)]


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("M,V", HEAD_SHAPES)
def test_head_top_vs_own_logits(engines, dtype, M, V):
    eng = engines(dtype)
    x, g, b, emb, targets, _ = _head_case(dtype, M, 64, V, 8100 + M + V)
    for k in (1, 3, 8):
        out, z, worst, n_hit = _check_head_top(eng, x, g, b, emb, targets, k)
        print(dtype, "M", M, "V", V, "k", k, "worst |error| / bound", worst, "targets among the k:", n_hit)
        n_cand = min(k, V)
        assert np.all(out["alt_id"][:, :n_cand] >= 0) and np.all(out["alt_id"][:, n_cand:] == -1)
        assert out["alt_id"][0, 0] == V - 1                       # _head_case's row 0: the column next to the padding wins


def _planted(dtype, seed=31):
    """M = 9, D = 64, V = 250 (four splits of one tile group, ragged last tile).  Row m's planted columns are multiples of its
    own normalised activation, so their logits in row m are the multipliers (50 .. 60) up to the 16-bit rounding of the
    embedding, far above what anything else reaches there."""
    M, D, V = 9, 64, 250
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((M, D)) * 1.5 + 0.3).astype(np.float32)
    g = (1.0 + 0.1 * rng.standard_normal(D)).astype(np.float32)
    b = (0.05 * rng.standard_normal(D)).astype(np.float32)
    emb = (rng.standard_normal((V, D)) * 0.02).astype(np.float32)
    a16, _ = _ln16(x, g, b, dtype)
    unit = lambda m: a16[m] / np.dot(a16[m], a16[m])
    plant = {0: [(3, 60), (19, 58), (35, 56), (51, 54)],                              # one lane's columns of one tile group
             1: [(10, 60), (70, 58), (130, 56), (200, 54)],                           # one best per split
             2: [(249, 60), (248, 59), (241, 58), (233, 57), (226, 56), (211, 55), (201, 54), (193, 53)],   # all in the last split
             4: [(40, 55), (100, 55), (180, 55)],                                      # identical rows in three splits
             5: [(5, 60), (6, 58), (65, 55), (112, 55)],                               # a tie inside one tile group (lanes 1, 0)
             6: [(7, 60), (8, 58), (30, 55), (150, 55)],                               # a tie across splits
             7: [(90, 60)]}                                                            # the target is the best
    for m, cols in plant.items():
        for n, s in cols:
            emb[n] = (unit(m) * float(s)).astype(np.float32)
    emb = _round16(emb, dtype)
    targets = rng.integers(0, V, M).astype(np.int32)
    targets[7] = 90
    return x, g, b, emb, targets, plant


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_head_top_planted_rows(engines, dtype):
    eng = engines(dtype)
    x, g, b, emb, targets, plant = _planted(dtype)
    for m in (4, 5, 6):                                           # the ties are exact: identical embedding rows
        assert np.array_equal(emb[plant[m][-1][0]], emb[plant[m][-2][0]])
    out8, z, worst, n_hit = _check_head_top(eng, x, g, b, emb, targets, 8)
    ids = out8["alt_id"]
    for m in (0, 1, 2, 4, 5, 6, 7):                               # the planted columns lead, in the planted order
        want = [n for n, _ in plant[m]]
        assert ids[m, :len(want)].tolist() == want, (m, ids[m].tolist())
    assert ids[7, 0] == targets[7] and 0 < n_hit < 9, n_hit        # a row whose target is among the k, and rows whose is not
    out3, _, _, _ = _check_head_top(eng, x, g, b, emb, targets, 3)
    assert out3["alt_id"][5, :3].tolist() == [5, 6, 65] and out3["alt_id"][6, :3].tolist() == [7, 8, 30]   # lower id in, higher out
    assert np.array_equal(out3["alt_id"][:, :3], ids[:, :3]) and np.array_equal(_bits(out3["alt_logprob"][:, :3]), _bits(out8["alt_logprob"][:, :3]))
    print(dtype, "planted rows: worst |error| / bound", worst)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_head_top_monotone_rows(engines, dtype):
    """Row 0 strictly descending in the id (nothing enters a list after its fill), row 1 = -row 0 strictly ascending (every column
    enters).  With a zero LayerNorm bias, x[1] = -x[0] gives a16[1] = -a16[0] exactly, so one embedding serves both."""
    eng = engines(dtype)
    D, V = 64, 250
    rng = np.random.default_rng(77)
    x0 = (rng.standard_normal(D) * 1.5).astype(np.float32)
    x = np.stack([x0, -x0])
    g = (1.0 + 0.1 * rng.standard_normal(D)).astype(np.float32)
    b = np.zeros(D, np.float32)
    a16, _ = _ln16(x, g, b, dtype)
    unit = a16[0] / np.dot(a16[0], a16[0])
    emb = _round16(np.stack([unit * (125.0 - 0.5 * n) for n in range(V)]).astype(np.float32), dtype)
    out, z, worst, _ = _check_head_top(eng, x, g, b, emb, np.asarray([0, V - 1], np.int32), 8)
    assert np.all(np.diff(z[0]) < 0) and np.all(np.diff(z[1]) > 0), "the case is not strictly monotone in this type"
    assert out["alt_id"][0].tolist() == list(range(8)) and out["alt_id"][1].tolist() == list(range(V - 1, V - 9, -1))
    print(dtype, "monotone rows: worst |error| / bound", worst)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_head_top_full_size(engines, dtype):
    eng = engines(dtype)
    x, g, b, emb, targets, _ = _head_case(dtype, 64, 1280, 51866, 99)
    out, z, worst, n_hit = _check_head_top(eng, x, g, b, emb, targets, 8)
    print(dtype, "M 64 D 1280 V 51866 k 8: worst |error| / bound", worst, "targets among the k:", n_hit)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("M,V", [(1, 250), (37, 250), (130, 250), (37, 51866)])
def test_head_stop_top(engines, dtype, M, V):
    eng = engines(dtype)
    x, g, b, emb, targets, _ = _head_case(dtype, M, 64, V, 9100 + M + V)
    for k in (1, 3, 8):
        out, z, worst, _ = _check_head_top(eng, x, g, b, emb, targets, k, stop=(V - 20, V - 10))
        print(dtype, "STOP M", M, "V", V, "k", k, "worst |error| / bound", worst)


def test_head_top_refusals(engines, tiny):
    eng = engines("bf16")
    x = np.zeros((2, 64), np.float32); emb = np.zeros((20, 64), np.float32); one = np.ones(64, np.float32)
    for k in (0, 9, -1):
        with pytest.raises(EngineError):
            eng.test_score_head_top(x, one, one, emb, [0, 1], k)
    with pytest.raises(EngineError):
        eng.test_score_head_top(x, one, one, emb, [0, 20], 3)
    with pytest.raises(EngineError):
        eng.set_score_top_logprobs(9)
    with pytest.raises(EngineError):
        eng.set_score_top_logprobs(-1)
    ids = np.zeros(8, np.int32); lp = np.zeros(8, np.float32)
    P = lambda a: a.ctypes.data_as(__import__("ctypes").c_void_p)
    assert eng.lib.cw_get_score_top_logprobs(eng.ctx, P(ids), P(lp), 1, 8) != 0          # off
    eng.set_score_top_logprobs(1)
    try:
        assert eng.lib.cw_get_score_top_logprobs(eng.ctx, P(ids), P(lp), 1, 8) != 0      # on, but no call has run
    finally:
        eng.set_score_top_logprobs(0)


# ------------------------------------------------------------------------------------------------------------ row kernel
def _rows_case(rows, V, seed):
    ldv = (V + 3) // 4 * 4
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((rows, ldv)) * 3.0).astype(np.float32)
    z[:, V:] = 100.0                                              # hot pad columns: they take no part
    z[0, V - 1] = 50.0
    if V > 5:
        z[0, [0, V // 2]] = 40.0                                  # an exact tie behind it: the lower id first
    if rows > 1:
        z[1, 1] = -np.inf
        z[2, :V] = -np.inf                                        # no candidate at all
        z[3, 2] = np.nan                                          # a NaN is no candidate (and makes the row's normaliser NaN)
        z[4, :V] = -np.inf; z[4, [V - 1, 0]] = [1.0, 1.0]         # two candidates, tied
        z[5, :V] = 0.25                                           # every column ties
    targets = rng.integers(0, V, rows).astype(np.int32)
    targets[0] = V - 1
    return z, targets


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("V", [5, 250, 51866])
@pytest.mark.parametrize("rows", [1, 8])
def test_rows_top_vs_float64(engines, dtype, V, rows):
    eng = engines(dtype)
    z, targets = _rows_case(rows, V, 600 + V + rows)
    for k in (1, 3, 8):
        for stop in (None, (V - 2, V - 1)):
            out = eng.test_score_rows_top(z, V, targets, k, stop=stop)
            problems, worst = R.check_topk(out["alt_id"], out["alt_logprob"], z, V, k, V / 256, R.ROWS_C)
            assert not problems, (k, stop, problems[:3])
            _identities(out, None, targets, k)
            assert out["alt_id"][0, 0] == V - 1 and (V == 5 or k < 3 or out["alt_id"][0, 1:3].tolist() == [0, V // 2])
            if rows > 1:
                assert np.all(out["alt_id"][2] == -1) and out["alt_id"][4, :2].tolist() == ([0, V - 1] if k > 1 else [0, -1])
                assert out["alt_id"][5, :k].tolist() == list(range(min(k, V)))[:k] + [-1] * max(0, k - V)
                assert np.all(out["alt_id"][3, :min(k, V - 1)] >= 0) and 2 not in out["alt_id"][3] and np.isnan(out["alt_logprob"][3]).all()
        print(dtype, "rows", rows, "V", V, "k", k, "worst |error| / bound", worst)
    if rows > 1:                                                  # STOP and plain forms: the same alternatives, bit for bit
        a = eng.test_score_rows_top(z, V, targets, 8)
        s = eng.test_score_rows_top(z, V, targets, 8, stop=(V - 2, V - 1))
        assert np.array_equal(a["alt_id"], s["alt_id"]) and np.array_equal(_bits(a["alt_logprob"]), _bits(s["alt_logprob"]))


# ---------------------------------------------------------------------------------------------------------------- engine
def _engine(spec, W, dtype, rows):
    e = Engine(spec, dtype=dtype, max_batch=rows)
    e.load_state_dict(W)
    return e


def _same_lists(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape
        if x.dtype.kind == "f":
            assert np.array_equal(_bits(x), _bits(y))
        else:
            assert np.array_equal(x, y)


def _alts_consistent(lp, ti, tl, ai, al, rows, k):
    for r in range(len(rows)):
        n = len(rows[r]) - 3
        assert ai[r].shape == (n, k) and al[r].shape == (n, k) and ai[r].dtype == np.int64 and al[r].dtype == np.float32
        assert np.array_equal(ai[r][:, 0], ti[r]) and np.array_equal(_bits(al[r][:, 0]), _bits(tl[r]))
        assert np.all(ai[r] >= 0) and np.all(np.diff(al[r].astype(np.float64), axis=1) <= 0)
        for j in range(n):
            assert len(set(ai[r][j].tolist())) == k
            w = np.flatnonzero(ai[r][j] == rows[r][3 + j])
            if w.size:
                assert _bits(al[r][j, w[0]:w[0] + 1])[0] == _bits(lp[r][j:j + 1])[0]


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_engine_calls_k8_against_k0(tiny, dtype):
    g, v, W, spec = tiny
    eng = _engine(spec, W, dtype, rows=33)
    try:
        for n_rows in (1, 9, 33):
            _, nf = eng.mel(_clips(n_rows))
            rows = _ragged_rows(v, spec, n_rows, 700 + n_rows, longest=(dtype != "f32" and n_rows == 9))
            off = eng.score_tokens(rows, 3)
            on = eng.score_tokens(rows, 3, top_logprobs=8)
            off2 = eng.score_tokens(rows, 3)
            assert len(off) == 3 and len(on) == 5
            for a, b_, c in zip(off, on[:3], off2):
                _same_lists(a, b_); _same_lists(a, c)
            _alts_consistent(*on, rows, 8)
            on3 = eng.score_tokens(rows, 3, top_logprobs=3)        # the first 3 of the 8
            for r in range(n_rows):
                assert np.array_equal(on3[3][r], on[3][r][:, :3]) and np.array_equal(_bits(on3[4][r]), _bits(on[4][r][:, :3]))
            if n_rows == 33:
                continue                                          # (the alignment calls: fewer rows are enough)
            a_off = eng.align_score_tokens(nf, rows, 3)
            a_on = eng.align_score_tokens(nf, rows, 3, top_logprobs=8)
            assert len(a_off) == 4 and len(a_on) == 6
            for a, b_ in zip(a_off, a_on[:4]):
                _same_lists(a, b_)
            if dtype != "f32":                                    # the prefill: the alignment capture changes no score
                _same_lists(a_on[4], on[3])
            _alts_consistent(*a_on[1:], rows, 8)
            Ns = [len(r) - 4 for r in rows]
            every = [np.ones(N + 1, bool) for N in Ns]
            forced = [r % 2 == 0 for r in range(n_rows)]
            c_off = eng.align_cut_tokens(nf, rows, 3, every, forced)
            c_on = eng.align_cut_tokens(nf, rows, 3, every, forced, top_logprobs=8)
            assert len(c_off) == 7 and len(c_on) == 9
            assert np.array_equal(c_off[0], c_on[0]) and np.array_equal(_bits(c_off[1]), _bits(c_on[1]))
            for a, b_ in zip(c_off[2:], c_on[2:7]):
                _same_lists(a, b_)
            _alts_consistent(c_on[3], c_on[5], c_on[6], c_on[7], c_on[8], rows, 8)
            _same_lists(c_on[7], a_on[4]); _same_lists(c_on[8], a_on[5])     # the STOP forms list the same alternatives
    finally:
        eng.close()


def test_switch_is_cleared_when_the_call_raises(tiny):
    g, v, W, spec = tiny
    eng = _engine(spec, W, "bf16", rows=2)
    try:
        eng.mel(_clips(1))
        init = [v.sot, v.lang_id("en"), v.transcribe]
        with pytest.raises(EngineError):
            eng.score_tokens([np.asarray(init + [5, v.eos, 6, v.eos])], 3, top_logprobs=4)      # eos inside
        ids = np.zeros(64, np.int32); lp = np.zeros(64, np.float32)
        P = lambda a: a.ctypes.data_as(__import__("ctypes").c_void_p)
        assert eng.lib.cw_get_score_top_logprobs(eng.ctx, P(ids), P(lp), 1, 6) != 0
        assert "off" in eng.lib.cw_last_error(eng.ctx).decode()
        with pytest.raises(ValueError):
            eng.score_tokens([np.asarray(init + [5, v.eos])], 3, top_logprobs=9)
        out = eng.score_tokens([np.asarray(init + [5, v.eos])], 3)
        assert len(out) == 3
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", ["bf16"])
def test_prefill_against_loop(tiny, dtype):
    g, v, W, spec = tiny
    eng = _engine(spec, W, dtype, rows=9)
    try:
        eng.mel(_clips(9))
        rows = _ragged_rows(v, spec, 9, 811, longest=False)
        eng.set_score_prefill(True)
        p = eng.score_tokens(rows, 3, top_logprobs=8)
        runs = eng.score_prefill_runs()
        eng.set_score_prefill(False)
        q = eng.score_tokens(rows, 3, top_logprobs=8)
        assert eng.score_prefill_runs() == runs
        _alts_consistent(*q, rows, 8)
        worst, common, total = 0.0, 0, 0
        for r in range(9):
            for j in range(len(p[3][r])):
                a = dict(zip(p[3][r][j].tolist(), p[4][r][j].tolist()))
                b_ = dict(zip(q[3][r][j].tolist(), q[4][r][j].tolist()))
                both = set(a) & set(b_)
                common += len(both); total += 8
                worst = max([worst] + [abs(a[i] - b_[i]) for i in both])
        print(dtype, "prefill vs loop: worst |difference| over", common, "of", total, "common alternatives:", worst)
        assert worst <= TOKEN_BOUND[dtype] and common >= total // 2
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_rows_per_item_independence(tiny, dtype):
    g, v, W, spec = tiny
    eng = _engine(spec, W, dtype, rows=16)
    try:
        clips = _clips(3, seed=70)
        cands = _ragged_rows(v, spec, 15, 5, longest=False)                   # 3 items x 5 candidates
        eng.mel(clips)
        five = eng.score_tokens(cands, 3, rows_per_item=5, top_logprobs=8)
        for item in range(3):
            eng.mel([clips[item]])
            k = item * 5 + 2
            one = eng.score_tokens([cands[k]], 3, rows_per_item=1, top_logprobs=8)
            if dtype == "f32":      # the loop's decode step picks kernels by batch size: equal within the f32 bound, not bit for bit
                for j in range(len(one[3][0])):
                    a = dict(zip(one[3][0][j].tolist(), one[4][0][j].tolist()))
                    b_ = dict(zip(five[3][k][j].tolist(), five[4][k][j].tolist()))
                    assert all(abs(a[i] - b_[i]) <= 4e-3 for i in set(a) & set(b_)) and len(set(a) & set(b_)) >= 4
            else:
                assert np.array_equal(one[3][0], five[3][k]) and np.array_equal(_bits(one[4][0]), _bits(five[4][k]))
    finally:
        eng.close()


# -------------------------------------------------------------------------------------------------------------- pipeline
def _check_tokens(toks, k):
    for t in toks:
        top = t["top_logprobs"]
        assert 1 <= len(top) <= k and all(set(e) == {"id", "text", "logprob"} for e in top)
        assert [e["logprob"] for e in top] == sorted((e["logprob"] for e in top), reverse=True)
        ids = [e["id"] for e in top]
        assert t["rank"] == (ids.index(t["id"]) if t["id"] in ids else None)
        if t["rank"] is not None:
            assert top[t["rank"]]["logprob"] == t["logprob"]
        else:
            assert t["logprob"] <= top[-1]["logprob"]


@pytest.mark.parametrize("dtype", ["bfloat16", "float32"])
def test_pipeline_score_align_align_long(tiny, dtype):
    g, v, W, spec = tiny
    pipe = cw.pipeline("automatic-speech-recognition", model=cw.ModelBundle(spec, W), tokenizer=collate.Vocabulary.from_synthetic(v),
                       batch_size=4, return_timestamps="word", torch_dtype=dtype, device="cuda:0")
    try:
        kw = dict(language="<|en|>", task="transcribe")
        short = syn.synth_audio(90, 16000 * 4, "mixed")
        text = [ord(c) for c in " abc def ghi"]
        plain = pipe.score(short, text, **kw)
        assert pipe.score(short, text, top_logprobs=0, **kw) == plain
        sc = pipe.score(short, text, top_logprobs=3, **kw)
        assert {k_: sc[k_] for k_ in ("text", "logprob", "avg_logprob", "chunks")} == {k_: plain[k_] for k_ in ("text", "logprob", "avg_logprob", "chunks")}
        assert [{k_: t[k_] for k_ in ("id", "logprob", "top_id", "top_logprob")} for t in sc["tokens"]] == plain["tokens"]
        _check_tokens(sc["tokens"], 3)
        assert all(t["top_logprobs"][0]["id"] == t["top_id"] and t["top_logprobs"][0]["logprob"] == t["top_logprob"] for t in sc["tokens"])
        # the lists are the engine's arrays
        eng = pipe.engine
        eng.mel([short])
        row = np.asarray([v.sot, v.lang_id("en"), v.transcribe] + text + [v.eos], np.int64)
        lp, ti, tl, ai, al = eng.score_tokens([row], 3, top_logprobs=3)
        assert [[e["id"] for e in t["top_logprobs"]] for t in sc["tokens"]] == ai[0].tolist()
        assert [[e["logprob"] for e in t["top_logprobs"]] for t in sc["tokens"]] == al[0].astype(np.float64).tolist()

        a_plain = pipe.align(short, text, return_scores=True, **kw)
        assert pipe.align(short, text, return_scores=True, top_logprobs=0, **kw) == a_plain
        al3 = pipe.align(short, text, return_scores=True, top_logprobs=3, **kw)
        assert [{k_: c[k_] for k_ in c if k_ != "tokens"} for c in al3["chunks"]] == a_plain["chunks"]
        flat = [t for c in al3["chunks"] for t in c["tokens"]]
        _check_tokens(flat, 3)
        assert [t["id"] for t in flat] == text                              # the collator's groups cover the transcript
        assert [t["top_logprobs"] for t in flat] == [t["top_logprobs"] for t in sc["tokens"][:-1]]
        assert [c["logprob"] for c in al3["chunks"]] == pytest.approx([sum(t["logprob"] for t in c["tokens"]) for c in al3["chunks"]], abs=1e-5)

        long_clip = syn.synth_audio(7, 16000 * 70, "mixed")
        ltext = [ord(c) for c in " abc" * 15]                                 # 60 tokens, 15 words, at most 16 per window
        l_plain = pipe.align_long(long_clip, ltext, return_scores=True, max_window_tokens=16, **kw)
        windows = len(pipe.stats["align_long"])
        assert pipe.align_long(long_clip, ltext, return_scores=True, top_logprobs=0, max_window_tokens=16, **kw) == l_plain
        l3 = pipe.align_long(long_clip, ltext, return_scores=True, top_logprobs=3, max_window_tokens=16, **kw)
        assert len(pipe.stats["align_long"]) == windows >= 3
        assert [{k_: c[k_] for k_ in c if k_ != "tokens"} for c in l3["chunks"]] == l_plain["chunks"]
        assert l3["logprob"] == l_plain["logprob"]
        flat = [t for c in l3["chunks"] for t in c["tokens"]]
        _check_tokens(flat, 3)
        assert [t["id"] for t in flat] == ltext                              # every kept token once, none from behind a cut
        print(dtype, "align_long:", windows, "windows,", len(l3["chunks"]), "chunks")
        for fn, args in ((pipe.align, (short, text)), (pipe.align_long, (long_clip, ltext))):
            with pytest.raises(ValueError):
                fn(*args, top_logprobs=3, **kw)                               # needs return_scores=True
            with pytest.raises(ValueError):
                fn(*args, return_scores=True, top_logprobs=9, **kw)
        with pytest.raises(ValueError):
            pipe.score(short, text, top_logprobs=True, **kw)
    finally:
        pipe.engine.close()
