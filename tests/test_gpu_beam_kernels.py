"""GPU tests of the beam-search candidate selection (csrc/elementwise.hip: beam_topk_partial_kernel + beam_topk_merge_kernel, the
default two-stage form, and beam_topk_kernel, the single-block form) against the float64 definition of tests/beam_refs.py, through
cw_test_beam_topk: the hook fills SampleParams with the function cw_beam_step uses and calls the same launcher, holds +75 in the
pad columns, 0xff bytes in the candidate buffers and 1e30 in every float of the slice records.

Ids must equal the reference exactly; values lie within the form's derived bound (beam_refs' module docstring); (-inf, -1) stands
exactly behind the last candidate; nothing behind nb * n_cand entries of the candidate buffers is written.  Every test prints its
worst |err| / bound.  tests/test_beam_refs.py proves on the CPU that this comparison rejects the planted faults."""
import numpy as np
import pytest

from crisperwhisper_amd import synthetic as syn
from crisperwhisper_amd.engine import Engine, EngineError
from tests import beam_refs as B
from tests import helpers as Hh

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "bf16", "f16"]
ONE_BLOCK = {"two_stage": 0, "single_block": 1}


@pytest.fixture(scope="module")
def engines():
    g, v, W, spec = Hh.tiny_setup()
    out = {dt: Engine(spec, dtype=dt, max_batch=15) for dt in DTYPES}
    yield out
    for e in out.values():
        e.lib.cw_test_set_option(b"beam_topk_1block", 0)
        e.close()


@pytest.fixture(scope="module")
def large():
    """The selection at the vocabulary of large-v3 (51 866 columns: 13 loads per thread, the last one ragged; the last slice is
    short and holds every timestamp), one layer, no weights -- as test_sample_kernel_large_vocab_vs_oracle builds it."""
    g, v = syn.large_v3_geometry()
    g.enc_layers = g.dec_layers = 1
    spec = syn.model_spec(g, v, n_align=1)
    spec.alignment_heads = [[0, 0]]
    eng = Engine(spec, dtype="bf16", max_batch=8)
    yield eng
    eng.lib.cw_test_set_option(b"beam_topk_1block", 0)
    eng.close()


def _form(eng, form):
    assert eng.lib.cw_test_set_option(b"beam_topk_1block", ONE_BLOCK[form]) == 0


def _launch(eng, rows, refs, sel, n_cand, form, what):
    """One launch on the table rows `sel` (they share t and min_new_tokens): everything asserted.  -> (ids, values, worst ratio)"""
    lg = np.stack([rows[i][2] for i in sel])
    ids = np.stack([rows[i][1] for i in sel])
    val, tok, untouched = eng.test_beam_topk(lg, ids, B.N_PROMPT, n_cand, min_new_tokens=rows[sel[0]][3])
    assert val.shape == tok.shape == (len(sel), n_cand) and val.dtype == np.float32 and tok.dtype == np.int32
    assert untouched, f"{what}: entries behind [{len(sel)}][{n_cand}] of the candidate buffers were written"
    worst, bad = 0.0, []
    for b, i in enumerate(sel):
        ok, w, why = B.compare(tok[b], val[b], refs[i], n_cand, form)
        worst = max(worst, w)
        if not ok:
            bad.append((rows[i][0], why))
    assert not bad, (what, bad[:3])
    return tok, val, worst


def _hot_then_narrow(eng, rows, refs, form, what):
    """An n_cand = 64 launch on the hottest rows, then an n_cand = 2 launch on other rows: with the poison fill in between, a record
    or a list entry of the earlier launch (values 40 and more) that was read again would win."""
    names = [r[0] for r in rows]
    hot = [names.index(n) for n in ("all_winners_in_the_text_slice", "all_winners_in_the_tb_slice", "raw_maximum_is_masked")]
    cold = [names.index(n) for n in ("five_allowed_tokens", "tie_in_ragged_tail/ts_low", "all_minus_inf")]
    assert len({len(rows[i][1]) for i in hot + cold}) == 1 and not any(rows[i][3] for i in hot + cold)
    w1 = _launch(eng, rows, refs, hot, 64, form, what + " hot rows")[2]
    w2 = _launch(eng, rows, refs, cold, 2, form, what + " after the hot rows")[2]
    return max(w1, w2)


@pytest.mark.parametrize("n_cand", [1, 2, 10, 64])
@pytest.mark.parametrize("form", list(ONE_BLOCK))
@pytest.mark.parametrize("dt", DTYPES)
def test_tiny_vocabulary_table(engines, dt, form, n_cand):
    """Every row of the tiny table alone, then in launches of up to 15 rows that share (t, min_new_tokens)."""
    rows, refs = B.table("tiny")
    eng = engines[dt]
    what = f"tiny {dt} {form} n_cand={n_cand}"
    _form(eng, form)
    try:
        worst = _hot_then_narrow(eng, rows, refs, form, what)
        alone = {}
        for i in range(len(rows)):
            tok, val, w = _launch(eng, rows, refs, [i], n_cand, form, what + " alone")
            alone[i] = (tok[0].tobytes(), val[0].tobytes())
            worst = max(worst, w)
        n = 0
        for sel in B.groups(rows, 15):
            tok, val, w = _launch(eng, rows, refs, sel, n_cand, form, what + " batched")
            worst = max(worst, w)
            for b, i in enumerate(sel):                           # a row's result does not depend on its neighbours
                assert (tok[b].tobytes(), val[b].tobytes()) == alone[i], (what, rows[i][0])
            n += len(sel)
        assert n == len(rows)
    finally:
        _form(eng, "two_stage")
    print(f"{what}: {len(rows)} rows, worst |err| / bound = {worst:.3f}")
    assert worst < 1.0


@pytest.mark.parametrize("n_cand", [10, 64])
@pytest.mark.parametrize("form", list(ONE_BLOCK))
def test_large_vocabulary_table(large, form, n_cand):
    """V = 51866, 8 rows per launch."""
    rows, refs = B.table("large")
    what = f"V=51866 bf16 {form} n_cand={n_cand}"
    _form(large, form)
    try:
        worst = _hot_then_narrow(large, rows, refs, form, what)
        n = 0
        for sel in B.groups(rows, 8):
            worst = max(worst, _launch(large, rows, refs, sel, n_cand, form, what)[2])
            n += len(sel)
        assert n == len(rows)
    finally:
        _form(large, "two_stage")
    print(f"{what}: {len(rows)} rows, worst |err| / bound = {worst:.3f}")
    assert worst < 1.0


def _both_forms(eng, which, size, n_cand, what):
    rows, refs = B.table(which)
    out, worst = {}, {}
    try:
        for form in ONE_BLOCK:
            _form(eng, form)
            res = [_launch(eng, rows, refs, sel, n_cand, form, f"{what} {form}") for sel in B.groups(rows, size)]
            out[form] = np.concatenate([r[0] for r in res])
            worst[form] = max(r[2] for r in res)
    finally:
        _form(eng, "two_stage")
    assert out["two_stage"].tobytes() == out["single_block"].tobytes()      # ids bit-identical; the values' reductions differ
    print(f"{what}: worst |err| / bound = " + ", ".join(f"{f} {w:.3f}" for f, w in worst.items()))
    assert max(worst.values()) < 1.0


@pytest.mark.parametrize("dt", DTYPES)
def test_both_forms_list_the_same_ids_tiny(engines, dt):
    _both_forms(engines[dt], "tiny", 15, 64, f"cross-form tiny {dt}")


def test_both_forms_list_the_same_ids_large(large):
    _both_forms(large, "large", 8, 64, "cross-form V=51866")


def test_the_hook_refuses_what_the_header_says(engines):
    g, v, W, spec = Hh.tiny_setup()
    rows, refs = B.table("tiny")
    eng = engines["f32"]
    V = spec.vocab_size
    sel = B.groups(rows, 15)[0]
    lg = np.stack([rows[i][2] for i in sel]); ids = np.stack([rows[i][1] for i in sel]).astype(np.int32)
    t = ids.shape[1]

    def raw(nb, lgp, idp, t_, n_prompt, mn, n_cand, vp=True, ip=True):
        val = np.zeros(eng.max_batch * 64, np.float32); tok = np.zeros(eng.max_batch * 64, np.int32)
        p = lambda a: None if a is None else a.ctypes.data_as(__import__("ctypes").c_void_p)
        eng._chk(eng.lib.cw_test_beam_topk(eng.ctx, nb, p(lgp), p(idp), t_, n_prompt, mn, n_cand, p(val if vp else None),
                                           p(tok if ip else None)))

    one_lg, one_id = np.ascontiguousarray(lg[:1]), np.ascontiguousarray(ids[:1])
    raw(1, one_lg, one_id, t, B.N_PROMPT, 0, 5)                                # the valid call the variants below break
    big_lg = np.zeros((16, V), np.float32); big_id = np.tile(one_id, (16, 1))
    bad_id = one_id.copy(); bad_id[0, -1] = V
    neg_id = one_id.copy(); neg_id[0, 0] = -1
    for kw in (dict(nb=0), dict(nb=16, lgp=big_lg, idp=big_id), dict(n_cand=0), dict(n_cand=65), dict(t_=B.N_PROMPT - 1),
               dict(t_=spec.max_target_positions), dict(n_prompt=0), dict(n_prompt=t + 1), dict(mn=-1), dict(idp=bad_id),
               dict(idp=neg_id), dict(lgp=None), dict(idp=None), dict(vp=False), dict(ip=False)):
        args = dict(nb=1, lgp=one_lg, idp=one_id, t_=t, n_prompt=B.N_PROMPT, mn=0, n_cand=5)
        args.update(kw)
        with pytest.raises(EngineError):
            raw(**args)
    # an open beam search: the hook would overwrite its state
    eng.load_state_dict(W)
    eng.mel([syn.synth_audio(5, 16000, "mixed")])
    eng.encode([0], [0], [3000])
    eng.beam_begin(np.array([[v.sot, v.lang_id("en"), v.transcribe]], np.int32), 5, 12)
    with pytest.raises(EngineError, match="beam search is open"):
        raw(1, one_lg, one_id, t, B.N_PROMPT, 0, 5)
    eng.beam_step(10)
    eng.beam_finish(np.zeros((1, 3), np.int32))
    # a valid call afterwards still passes
    _launch(eng, rows, refs, sel, 10, "two_stage", "after the refusals")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_beam_finish_gathers_alignment_rows_by_beam(dt):
    """align_gather_kernel through the public ABI: 3 items x 5 beams, 12 steps with scripted parents; the alignment rows read
    right before cw_beam_finish (on bf16: the un-normalised capture through align_normalize) against the rows read after it,
    G[i, a, p] == A[row_of_pos[i, p], a, p] bit for bit, with a row_of_pos that changes row at every position and uses every
    beam.  The rows of A are finite and sum to 1, so an all-zero buffer cannot pass."""
    g, v, W, spec = Hh.tiny_setup()
    items, K, steps = 3, 5, 12
    R = items * K
    rng = np.random.default_rng(23)
    eng = Engine(spec, dtype=dt, max_batch=R)
    try:
        eng.load_state_dict(W)
        eng.mel([syn.synth_audio(80 + i, 160000, "mixed") for i in range(items)])
        eng.encode(list(range(items)), [0] * items, [3000] * items)
        prompt = np.array([[v.sot, v.lang_id("en"), v.transcribe]] * items, np.int32)
        n_prompt = prompt.shape[1]
        eng.beam_begin(prompt, K, n_prompt + steps + 4)
        for step in range(steps):
            vals, toks = eng.beam_step(2 * K)
            assert vals.shape == (R, 2 * K) and np.isfinite(vals[:, 0]).all()
            par = np.concatenate([i * K + (rng.permutation(K) if step % 3 else rng.integers(0, K, K)) for i in range(items)])
            col = (np.arange(R) + step) % (2 * K)             # every row takes another candidate: the beams of an item diverge
            tok = np.where(toks[par, col] >= 0, toks[par, col], ord("a") + np.arange(R) % K)
            eng.beam_advance(par.astype(np.int32), tok.astype(np.int32))
        L = n_prompt - 1 + steps
        Ha = len(spec.alignment_heads)
        A = eng.alignment(R, L)
        assert A.shape == (R, Ha, L, A.shape[3]) and np.isfinite(A).all()
        assert np.abs(A.astype(np.float64).sum(-1) - 1.0).max() < 1e-5
        row_of_pos = np.array([[i * K + (p + i) % K for p in range(L)] for i in range(items)], np.int32)
        assert all(len(set(r.tolist())) == K for r in row_of_pos) and (np.diff(row_of_pos, axis=1) != 0).all()
        eng.beam_finish(row_of_pos)
        G = eng.alignment(items, L)
        want = np.stack([np.stack([A[row_of_pos[i, p], :, p] for p in range(L)], axis=1) for i in range(items)])
        assert G.shape == want.shape and G.tobytes() == want.tobytes(), np.argwhere(G != want)[:5].tolist()
        # rows of different beams do differ, so a gather that ignored row_of_pos would be seen
        last = A[:, :, L - 1].reshape(items, K, -1)
        assert all(not np.array_equal(last[i, a], last[i, b]) for i in range(items) for a in range(K) for b in range(a))
    finally:
        eng.close()
